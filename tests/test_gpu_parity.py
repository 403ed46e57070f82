"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against
the oracle on the same seeded inputs — bit-exact, because everything on this path is 8-bit integer
arithmetic (no float exists on the reference path)."""
import ctypes
import hashlib
import json
import subprocess
import sys
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import LayerDesc, eight_layer_descs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
HASHES = json.loads((GOLDEN / "appendix_a_hashes.json").read_text())
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import api as _api
    return _api


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_mk_desc = LayerDesc.make


def _rand_params(rng, d):
    W = rng.integers(-8, 8, (d.OFM_CH, 5, 5, d.IFM_CH)).astype(np.int8)
    b = rng.integers(-128, 128, d.OFM_CH).astype(np.int8)
    return W, b, sicn_ref.pack_finn_tiles(W, d.SIMD, d.PE)


def _run_layer(api, d, words, b, x_np, **options):
    """options: sicn_options fields (per call; the library keeps no process-wide knobs)."""
    fpw = api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, words)
    fn = api.deconv522 if d.transposed else api.conv2d
    out = fn(d, fpw, b, _dev(x_np), None, x_np.shape[0], options=options or None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# (cin, cout, simd, pe, w, h, transposed) — every kernel family, odd sizes, sizes that are not a
# multiple of the 8x32 tile, single-row / single-column images, pixels >= 128 on the RGB layer.
SPECIAL = [
    (3, 128, 3, 8, 70, 38, 0), (3, 128, 3, 8, 5, 3, 0), (3, 128, 3, 8, 129, 17, 0), (3, 128, 1, 128, 64, 2, 0),
    (128, 128, 8, 16, 66, 18, 0), (128, 128, 8, 16, 7, 5, 0), (128, 128, 8, 16, 1, 1, 0), (128, 128, 4, 32, 131, 33, 0),
    (128, 192, 8, 24, 40, 22, 0), (128, 192, 8, 24, 65, 3, 0),
    (192, 128, 12, 16, 33, 9, 1), (192, 128, 12, 16, 3, 2, 1), (192, 128, 12, 16, 70, 17, 1),
    (128, 128, 8, 16, 34, 10, 1), (128, 128, 8, 16, 1, 1, 1), (128, 128, 8, 16, 65, 19, 1),
    (128, 3, 8, 3, 35, 11, 1), (128, 3, 8, 3, 1, 1, 1), (128, 3, 8, 3, 70, 9, 1), (128, 3, 16, 1, 33, 8, 1),
]
GENERIC = [(3, 8, 3, 4, 20, 12, 0), (6, 6, 2, 3, 13, 9, 0), (4, 12, 4, 6, 7, 5, 1), (12, 3, 12, 3, 9, 11, 1),
           (64, 32, 8, 8, 17, 6, 0), (32, 64, 8, 8, 6, 9, 1)]


@pytest.mark.parametrize("case", SPECIAL + GENERIC)
def test_layer_matches_oracle_random_weights(api, case):
    rng = np.random.default_rng(abs(hash(case)) % (1 << 32))
    d = _mk_desc(*case)
    W, b, words = _rand_params(rng, d)
    n = 2
    x = rng.integers(0, 256 if d.IFM_CH == 3 else 128, (n,) + d.in_shape, dtype=np.uint8)
    if d.IFM_CH != 3:
        x[0].reshape(-1)[:: 7] |= 0x80        # values the net never produces must still be exact mod 256
    got = _run_layer(api, d, words, b, x)
    ref_fn = sicn_ref.deconv522_ref if d.transposed else sicn_ref.conv2d_ref
    for i in range(n):
        ref = ref_fn(x[i], W, b)
        assert got[i].shape == ref.shape
        assert np.array_equal(got[i], ref), f"image {i}: {np.count_nonzero(got[i] != ref)} bytes differ"
    # and the stage-by-stage dataflow port agrees on the first image when it is small
    if d.algorithmic_macs < 4e8:
        assert np.array_equal(got[0], c_oracle.run_layer(d, words, b, x[0], "dataflow_im2col"))


@pytest.mark.parametrize("chunks", ["1", "2", "5"])
@pytest.mark.parametrize("case", [(3, 128, 3, 8, 140, 150, 0), (128, 3, 8, 3, 70, 45, 1), (128, 3, 8, 3, 64, 32, 1)])
def test_strip_kernels_long_strips(api, case, chunks):
    """L0 / L7 walk a vertical strip per workgroup (L7 through a rolling LDS window); force long strips
    on small images so that ring wrap-around, chunk boundaries and the last partial step are covered."""
    rng = np.random.default_rng(abs(hash(case)) % (1 << 32))
    d = _mk_desc(*case)
    W, b, words = _rand_params(rng, d)
    x = rng.integers(0, 256 if d.IFM_CH == 3 else 128, (2,) + d.in_shape, dtype=np.uint8)
    got = _run_layer(api, d, words, b, x, strip_chunks=int(chunks))
    ref_fn = sicn_ref.deconv522_ref if d.transposed else sicn_ref.conv2d_ref
    for i in range(2):
        ref = ref_fn(x[i], W, b)
        assert np.array_equal(got[i], ref), f"image {i}: {np.count_nonzero(got[i] != ref)} bytes differ"


MFMA_CASES = [c for c in SPECIAL if c[0] != 3 and c[1] != 3]


@pytest.mark.parametrize("prefetch", [1, 2])
@pytest.mark.parametrize("tile_x", ["16", "32"])
@pytest.mark.parametrize("case", MFMA_CASES + [(128, 128, 8, 16, 50, 20, 0), (192, 128, 12, 16, 37, 21, 1), (128, 192, 8, 24, 47, 18, 0),
                                  (192, 128, 12, 16, 45, 19, 0), (128, 192, 8, 24, 21, 13, 1), (192, 128, 12, 16, 9, 40, 0)])
def test_both_tile_widths_match_oracle(api, case, tile_x, prefetch):
    """The software-pipelined 16x16x64 kernels (k_mfma16p.hip) exist for 8 x 16 position tiles on every shape and for 8 x 32
    tiles on the 128 -> 128 shapes (the launcher picks by layer shape and grid size; tile_x = 32 on a 192-channel shape still
    gets 8 x 16); force each width on every shape, incl. the hyperprior stacks' conv 192 -> 128 and deconv 128 -> 192.
    prefetch = 1 and 2 both keep the automatic wide form out; 1 selected the plain kernels until they were removed and must
    now run exactly the pipelined ones."""
    rng = np.random.default_rng(abs(hash(case)) % (1 << 31) + int(tile_x))
    d = _mk_desc(*case)
    W, b, words = _rand_params(rng, d)
    x = rng.integers(0, 128, (2,) + d.in_shape, dtype=np.uint8)
    got = _run_layer(api, d, words, b, x, tile_x=int(tile_x), prefetch=prefetch)
    ref_fn = sicn_ref.deconv522_ref if d.transposed else sicn_ref.conv2d_ref
    for i in range(2):
        assert np.array_equal(got[i], ref_fn(x[i], W, b))


@pytest.mark.parametrize("split_n", [1, 2])
@pytest.mark.parametrize("case", MFMA_CASES + [(128, 128, 8, 16, 50, 20, 0), (192, 128, 12, 16, 37, 21, 1), (128, 192, 8, 24, 47, 18, 0),
                                  (192, 128, 12, 16, 45, 19, 0), (128, 192, 8, 24, 21, 13, 1), (128, 128, 8, 16, 33, 9, 1)])
def test_output_channel_split_matches_oracle(api, case, split_n):
    """On grids smaller than the chip the pipelined kernels split a layer's output channels over 2 / 3 workgroups of 64
    (sicn_options.split_n: 0 = by grid size, 1 = never, > 1 = always): both forms on every MFMA shape."""
    rng = np.random.default_rng(abs(hash(case)) % (1 << 31) + 77 * split_n)
    d = _mk_desc(*case)
    W, b, words = _rand_params(rng, d)
    x = rng.integers(0, 128, (3,) + d.in_shape, dtype=np.uint8)
    x[1].reshape(-1)[::5] |= 0x80
    got = _run_layer(api, d, words, b, x, tile_x=16, split_n=split_n)
    ref_fn = sicn_ref.deconv522_ref if d.transposed else sicn_ref.conv2d_ref
    for i in range(3):
        ref = ref_fn(x[i], W, b)
        assert np.array_equal(got[i], ref), (i, np.count_nonzero(got[i] != ref))


@pytest.mark.parametrize("split_n", [1, 2])
def test_output_channel_split_in_chain(api, split_n):
    xin = _dev(_input("rng768")[None])
    net = api.EightLayersNet(768, 512, options={"tile_x": 16, "split_n": split_n})
    out, latent = net.forward(xin)
    torch.cuda.synchronize()
    assert _sha(out[0].cpu().numpy()) == HASHES["layers"]["rng768"][7]
    assert _sha(latent[0].cpu().numpy()) == HASHES["layers"]["rng768"][3]


@pytest.mark.parametrize("grid", [8, 16, 24])
@pytest.mark.parametrize("case", [(128, 128, 8, 16, 512, 200, 0), (128, 128, 8, 16, 250, 104, 1)])
def test_wide_kernels_dynamic_tile_deal_matches_oracle(api, case, grid):
    """Round 5: inside a net (whose workspace carries the deal area) a wide persistent workgroup takes its tiles beyond the first two from
    ticket counters — its own XCD's, then the other XCDs' (k_mfma16x.hip: DealX).  Forced onto few workgroups (1 / 2 / 3 per XCD) that
    walk >= 16 tiles each, so that ranges run dry at different times and tickets are taken from other XCDs: every tile must be computed
    exactly once (any lost or doubled tile shows in the bytes), on repeated calls (the deal area is re-zeroed by every forward pass) and
    in a captured graph (the zeroing is a node of it); against the oracle and against the static deal (a layer call without a net)."""
    rng = np.random.default_rng(abs(hash(case)) % (1 << 31) + grid)
    d = _mk_desc(*case)
    W, b, words = _rand_params(rng, d)
    x = rng.integers(0, 128, (3,) + d.in_shape, dtype=np.uint8)
    x[1].reshape(-1)[::7] |= 0x80
    fpw = api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, words)
    net = api.EightLayersNet(descs=[d], params=[(fpw, b)], options={"wave_tile": 128, "persistent_grid": grid})
    xin = _dev(x)
    ref_fn = sicn_ref.deconv522_ref if d.transposed else sicn_ref.conv2d_ref
    ref = np.stack([ref_fn(x[i], W, b) for i in range(3)])
    for _ in range(3):
        out, _ = net.run_layers(0, 0, xin)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref)
    static = _run_layer(api, d, words, b, x, wave_tile=128, persistent_grid=grid)      # no workspace: the static deal
    assert np.array_equal(static, ref)
    out = torch.zeros_like(out)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            net.run_layers(0, 0, xin, out=out)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref)


def test_wide_kernels_fall_back_to_the_static_deal_in_a_workspace_of_the_old_size(api):
    """include/sicn.h: a workspace without room for the deal words (a size computed by library 0.2: 528 eight-byte words per layer less) is
    not an error — the wide kernels then deal every tile statically.  Same bytes either way."""
    import ctypes
    L = api._lib.lib()
    rng = np.random.default_rng(91)
    d = _mk_desc(128, 128, 8, 16, 250, 104, 1)           # 8 x 7 tiles x 3 images on 8 workgroups: 21 each, the deal's dynamic part is on
    W, b, words = _rand_params(rng, d)
    x = rng.integers(0, 128, (3,) + d.in_shape, dtype=np.uint8)
    fpw = api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, words)
    net = api.EightLayersNet(descs=[d], params=[(fpw, b)], options={"wave_tile": 128, "persistent_grid": 8})
    xin = _dev(x)
    full = int(L.sicn_net_workspace_bytes(net._h, 3))
    small = full - (528 * 8 + 255) // 256 * 256          # one layer's deal words, as sicn_abi.hip aligns them
    assert small >= 0                                     # (a one-layer net needs nothing else: 0 bytes then)
    ref = np.stack([sicn_ref.deconv522_ref(x[i], W, b) for i in range(3)])
    for nbytes in (full, small):
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")
        out = torch.zeros((3,) + d.out_shape, dtype=torch.uint8, device="cuda")
        rc = L.sicn_net_forward(net._h, 0, 0, ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), -1, None, 3,
                                ctypes.c_void_p(ws.data_ptr()), nbytes, api._stream_ptr(None))
        torch.cuda.synchronize()
        assert rc == 0 and np.array_equal(out.cpu().numpy(), ref), nbytes


PERSISTENT_CASES = [(128, 128, 8, 16, 130, 66, 0), (128, 128, 8, 16, 66, 18, 0), (128, 128, 8, 16, 7, 5, 0), (128, 128, 4, 32, 131, 33, 0),
                    (128, 128, 8, 16, 200, 90, 0), (128, 128, 8, 16, 64, 16, 0)]


@pytest.mark.parametrize("grid", [8, 16, 0])
@pytest.mark.parametrize("case", PERSISTENT_CASES)
def test_persistent_conv_matches_oracle(api, case, grid):
    """conv 128 -> 128 by PERSISTENT workgroups that walk through many tiles (k_conv_x: the plane refresh of a tile's last
    passes fetches the next tile, the weight ring wraps, the accumulator hand-over sits in the next tile's first pass).  Forced
    (wave_tile = 128) with 8 / 16 workgroups so that every one of them gets several tiles of these small inputs — across image
    boundaries (n = 3), ragged right / bottom tiles, single-tile images — and with the default grid."""
    rng = np.random.default_rng(abs(hash(case)) % (1 << 31) + grid)
    d = _mk_desc(*case)
    W, b, words = _rand_params(rng, d)
    x = rng.integers(0, 128, (3,) + d.in_shape, dtype=np.uint8)
    x[0].reshape(-1)[::7] |= 0x80
    got = _run_layer(api, d, words, b, x, wave_tile=128, persistent_grid=grid)
    for i in range(3):
        ref = sicn_ref.conv2d_ref(x[i], W, b)
        assert np.array_equal(got[i], ref), (i, np.count_nonzero(got[i] != ref))


@pytest.mark.parametrize("grid", [8, 40])
def test_persistent_conv_in_chain(api, grid):
    xin = _dev(np.stack([_input("rng768"), _input("ones768")]))
    net = api.EightLayersNet(768, 512, options={"wave_tile": 128, "persistent_grid": grid})
    out, latent = net.forward(xin)
    torch.cuda.synchronize()
    for i, name in enumerate(("rng768", "ones768")):
        assert _sha(out[i].cpu().numpy()) == HASHES["layers"][name][7]
        assert _sha(latent[i].cpu().numpy()) == HASHES["layers"][name][3]


WIDE_CASES = [(128, 128, 8, 16, 66, 18, 0), (128, 128, 8, 16, 7, 5, 0), (128, 128, 8, 16, 1, 1, 0), (128, 128, 4, 32, 131, 33, 0),
              (128, 128, 8, 16, 50, 20, 0), (128, 128, 8, 16, 200, 90, 0), (128, 128, 8, 16, 129, 67, 0), (128, 128, 8, 16, 300, 260, 0)]


@pytest.mark.parametrize("wave_tile,grid", [(64, 0), (128, 0), (128, 8), (128, 16)])
@pytest.mark.parametrize("case", WIDE_CASES)
def test_wide_wave_tile_conv_matches_oracle(api, case, wave_tile, grid):
    """conv 128 -> 128 exists in two forms: 64 x 128 outputs per wave at two waves per SIMD (k_mfma16p.hip) and
    128 x 128 per wave with AGPR-pinned accumulators at one wave per SIMD, by PERSISTENT workgroups that walk through 16 x 32
    tiles (k_mfma16x.hip, the default on full-size grids).  Force each on odd sizes, single pixels, several tiles, pixels with
    the high bit; the persistent form also with 8 / 16 workgroups, so that every one of them walks through several tiles —
    across image boundaries (n = 3), ragged right / bottom tiles, single-tile images."""
    rng = np.random.default_rng(abs(hash(case)) % (1 << 31) + wave_tile + grid)
    d = _mk_desc(*case)
    W, b, words = _rand_params(rng, d)
    x = rng.integers(0, 128, (3,) + d.in_shape, dtype=np.uint8)
    x[0].reshape(-1)[::7] |= 0x80
    got = _run_layer(api, d, words, b, x, tile_x=32, wave_tile=wave_tile, prefetch=1, persistent_grid=grid)
    for i in range(3):
        assert np.array_equal(got[i], sicn_ref.conv2d_ref(x[i], W, b)), (i, np.count_nonzero(got[i] != sicn_ref.conv2d_ref(x[i], W, b)))


WIDE_DECONV_CASES = [(128, 128, 8, 16, 34, 10, 1), (128, 128, 8, 16, 1, 1, 1), (128, 128, 8, 16, 65, 19, 1), (128, 128, 8, 16, 100, 45, 1),
                     (128, 128, 4, 32, 33, 17, 1), (128, 128, 8, 16, 7, 5, 1), (128, 128, 8, 16, 150, 130, 1)]


@pytest.mark.parametrize("grid", [0, 8, 16])
@pytest.mark.parametrize("case", WIDE_DECONV_CASES)
def test_wide_wave_tile_deconv_matches_oracle(api, case, grid):
    """deconv 128 -> 128 in the wide persistent form (k_deconv_x): 4 phases per tile with the accumulator hand-over woven into the
    next phase's first pass, the patch's two channel-group pairs in three rotating buffers; with 8 / 16 workgroups every one of
    them walks through several tiles (n = 3 images, ragged tiles, single pixels), so every buffer rotation is exercised."""
    rng = np.random.default_rng(abs(hash(case)) % (1 << 31) + grid)
    d = _mk_desc(*case)
    W, b, words = _rand_params(rng, d)
    x = rng.integers(0, 128, (3,) + d.in_shape, dtype=np.uint8)
    x[0].reshape(-1)[::7] |= 0x80
    got = _run_layer(api, d, words, b, x, tile_x=32, wave_tile=128, persistent_grid=grid)
    for i in range(3):
        ref = sicn_ref.deconv522_ref(x[i], W, b)
        assert np.array_equal(got[i], ref), (i, np.count_nonzero(got[i] != ref))


@pytest.mark.parametrize("wave_tile,grid", [(64, 0), (128, 0), (128, 8)])
def test_wide_wave_tile_in_chain(api, wave_tile, grid):
    xin = _dev(_input("rng768")[None])
    net = api.EightLayersNet(768, 512, options={"tile_x": 32, "wave_tile": wave_tile, "prefetch": 1, "persistent_grid": grid})
    out, latent = net.forward(xin)
    torch.cuda.synchronize()
    assert _sha(out[0].cpu().numpy()) == HASHES["layers"]["rng768"][7]
    assert _sha(latent[0].cpu().numpy()) == HASHES["layers"]["rng768"][3]


PIPE_CASES = [(128, 128, 8, 16, 34, 10, 1), (128, 128, 8, 16, 1, 1, 1), (128, 128, 8, 16, 65, 19, 1), (128, 128, 8, 16, 100, 45, 1),
              (128, 128, 4, 32, 33, 17, 1)]


@pytest.mark.parametrize("prefetch", [1, 2])
@pytest.mark.parametrize("case", PIPE_CASES + WIDE_CASES)
def test_pipelined_kernels_match_oracle(api, case, prefetch):
    """conv / deconv 128 -> 128 on the software-pipelined k_mfma16p.hip (prefetch = 1 | 2: never the automatic wide form; 1 selected
    the plain kernels until they were removed), with the 8 x 32 tile, on odd sizes / single pixels / several tiles / high-bit
    inputs."""
    rng = np.random.default_rng(abs(hash(case)) % (1 << 31) + prefetch)
    d = _mk_desc(*case)
    W, b, words = _rand_params(rng, d)
    x = rng.integers(0, 128, (3,) + d.in_shape, dtype=np.uint8)
    x[0].reshape(-1)[::7] |= 0x80
    got = _run_layer(api, d, words, b, x, tile_x=32, prefetch=prefetch)
    for i in range(3):
        ref = (sicn_ref.deconv522_ref if d.transposed else sicn_ref.conv2d_ref)(x[i], W, b)
        assert np.array_equal(got[i], ref), (i, np.count_nonzero(got[i] != ref))


@pytest.mark.parametrize("prefetch", [1, 2])
def test_pipelined_kernels_in_chain(api, prefetch):
    xin = _dev(_input("rng768")[None])
    net = api.EightLayersNet(768, 512, options={"tile_x": 32, "prefetch": prefetch})
    out, latent = net.forward(xin)
    torch.cuda.synchronize()
    assert _sha(out[0].cpu().numpy()) == HASHES["layers"]["rng768"][7]
    assert _sha(latent[0].cpu().numpy()) == HASHES["layers"]["rng768"][3]


@pytest.mark.parametrize("tile_x", ["16", "32"])
def test_both_tile_widths_in_chain(api, tile_x):
    xin = _dev(_input("rng768")[None])
    net = api.EightLayersNet(768, 512, options={"tile_x": int(tile_x)})
    out, latent = net.forward(xin)
    torch.cuda.synchronize()
    assert _sha(out[0].cpu().numpy()) == HASHES["layers"]["rng768"][7]
    assert _sha(latent[0].cpu().numpy()) == HASHES["layers"]["rng768"][3]


def test_specialised_and_generic_kernels_agree(api):
    from simple_image_compression_network_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(7)
    for case in [(3, 128, 3, 8, 70, 38, 0), (128, 128, 8, 16, 66, 18, 0), (128, 128, 8, 16, 34, 10, 1),
                 (128, 3, 8, 3, 35, 11, 1)]:
        d = _mk_desc(*case)
        _, b, words = _rand_params(rng, d)
        x = rng.integers(0, 128, (1,) + d.in_shape, dtype=np.uint8)
        assert L.sicn_kernel_for(ctypes.byref(d.to_c())) != b"generic"
        fast = _run_layer(api, d, words, b, x)
        slow = _run_layer(api, d, words, b, x, force_generic=1)     # per call: no process-wide switch exists
        assert L.sicn_kernel_for(ctypes.byref(d.to_c())) != b"generic"
        assert np.array_equal(fast, slow)


def test_two_streams_one_net_with_profiling(api):
    """sicn.h: handles are immutable, launches on different streams (and host threads) may run concurrently, each
    with its own workspace; the profiling ring hands out slots atomically. Two host threads drive two streams through
    ONE net handle with profiling on; every result must be exact and every launch must be accounted for."""
    import threading
    net = api.EightLayersNet(256, 256)
    net.profile(True)
    rng = np.random.default_rng(5)
    xs = [_dev(rng.integers(0, 256, (2, 256, 256, 3), dtype=np.uint8)) for _ in range(2)]
    ref = [net.forward(x)[0].clone() for x in xs]
    torch.cuda.synchronize()
    net.layer_ms(reset=True)
    L = api._lib.lib()
    nbytes = L.sicn_net_workspace_bytes(net._h, 2)
    ws = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(2)]
    outs = [torch.empty_like(ref[0]) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    iters, errs = 40, []

    def worker(k):
        try:
            for _ in range(iters):
                rc = L.sicn_eight_layers_net(net._h, ctypes.c_void_p(xs[k].data_ptr()), ctypes.c_void_p(outs[k].data_ptr()),
                                             None, 2, ctypes.c_void_p(ws[k].data_ptr()), nbytes,
                                             ctypes.c_void_p(streams[k].cuda_stream))
                if rc:
                    errs.append(rc)
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    torch.cuda.synchronize()
    assert not errs
    assert torch.equal(outs[0], ref[0]) and torch.equal(outs[1], ref[1])
    ms, cnt = net.layer_ms(reset=True)
    assert cnt == [2 * iters] * 8 and all(m > 0 for m in ms)
    net.profile(False)


def _input(name):
    if name == "ones768":
        return np.ones((512, 768, 3), np.uint8)
    if name == "rng768":
        return np.random.default_rng(0).integers(0, 256, (512, 768, 3), dtype=np.uint8)
    return np.random.default_rng(0).integers(0, 256, (256, 256, 3), dtype=np.uint8)


@pytest.mark.parametrize("name", ["rng256", "ones768", "rng768"])
def test_eight_layers_net_matches_reference_hashes(api, name):
    """All 8 layer outputs against SURVEY.md Appendix A (the reference's own templates, PARAM weights):
    BASELINE configs 1 (layer 0 of ones768) and 2 (rng256 analysis) are rows of this table."""
    x = _input(name)
    net = api.EightLayersNet(x.shape[1], x.shape[0])
    xin = _dev(x[None])
    got = []
    cur = xin
    for l in range(8):                               # layer by layer through sicn_net_forward
        cur, _ = net.run_layers(l, l, cur)
        got.append(_sha(cur[0].cpu().numpy()))
    assert got == HASHES["layers"][name]
    out, latent = net.forward(xin)                   # and in one call, with the latent tap
    torch.cuda.synchronize()
    assert _sha(out[0].cpu().numpy()) == HASHES["layers"][name][7]
    assert _sha(latent[0].cpu().numpy()) == HASHES["layers"][name][3]


def test_reference_entry_points(api):
    """conv2d_layer0 / deconv2d_layer4 / eight_layers_net with the reference's argument order."""
    x = _input("rng256")
    xin = _dev(x[None])
    l0 = api.conv2d_layer0(xin, None, 1)
    rec = api.eight_layers_net(xin, None, 1)
    net = api.EightLayersNet(256, 256)
    _, latent = net.forward(xin)
    l4 = api.deconv2d_layer4(latent, None, 1)
    torch.cuda.synchronize()
    assert _sha(l0[0].cpu().numpy()) == HASHES["layers"]["rng256"][0]
    assert _sha(l4[0].cpu().numpy()) == HASHES["layers"]["rng256"][4]
    assert _sha(rec[0].cpu().numpy()) == HASHES["layers"]["rng256"][7]


def test_1080p_full_net_matches_closed_form(api, param_closed_form):
    """BASELINE config 3: 1920x1080 -> latent 120x68x192 -> 1920x1088 reconstruction."""
    x = np.random.default_rng(0).integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    net = api.EightLayersNet(1920, 1080)
    out, latent = net.forward(_dev(x[None]))
    torch.cuda.synchronize()
    ref = sicn_ref.eight_layers_net_ref(x, param_closed_form)
    assert tuple(out.shape) == (1, 1088, 1920, 3) and tuple(latent.shape) == (1, 68, 120, 192)
    assert np.array_equal(latent[0].cpu().numpy(), ref[3])
    assert np.array_equal(out[0].cpu().numpy(), ref[7])


def _check_window(d, words, b, xin, yout, rng):
    """Oracle check of one random window of a full-size layer: run the C closed form on an input crop
    and compare the part of its output whose receptive field lies inside the crop (or at a true
    image edge, where the crop's zero padding IS the layer's padding)."""
    H, Wd = d.IFM_COL, d.IFM_ROW
    ch, cw = min(H, 24), min(Wd, 40)
    ch -= ch % 2
    cw -= cw % 2
    y0 = int(rng.integers(0, (H - ch) // 2 + 1)) * 2
    x0 = int(rng.integers(0, (Wd - cw) // 2 + 1)) * 2
    crop = np.ascontiguousarray(xin[y0:y0 + ch, x0:x0 + cw])
    ow, oh = (2 * cw, 2 * ch) if d.transposed else ((cw + 1) // 2, (ch + 1) // 2)
    dc = replace(d, IFM_ROW=cw, IFM_COL=ch, OFM_ROW=ow, OFM_COL=oh)
    ref = c_oracle.run_layer(dc, words, b, crop, "direct")
    s = 2 if d.transposed else 1          # output border that sees the crop's artificial padding
    f = 2.0 if d.transposed else 0.5
    t0 = 0 if y0 == 0 else s
    l0 = 0 if x0 == 0 else s
    t1 = oh if y0 + ch == H else oh - s
    l1 = ow if x0 + cw == Wd else ow - s
    oy0, ox0 = int(y0 * f), int(x0 * f)
    got = yout[oy0 + t0:oy0 + t1, ox0 + l0:ox0 + l1]
    assert np.array_equal(got, ref[t0:t1, l0:l1])


def test_4k_batch_windows_and_properties(api, param_words):
    """BASELINE config 4 shape on one GPU: 2 x (3840x2160) through all 8 layers.  The oracle cannot
    run 4K in seconds, so: (a) every layer is checked against the oracle on random windows, fed with
    the GPU's own previous-layer output; (b) batch independence: image 1 alone == image 1 in the
    batch; (c) a checksum of every layer is reproducible across two runs."""
    rng = np.random.default_rng(4)
    x = rng.integers(0, 256, (2, 2160, 3840, 3), dtype=np.uint8)
    net = api.EightLayersNet(3840, 2160)
    cur = _dev(x)
    sums = []
    for l, d in enumerate(net.descs):
        nxt, _ = net.run_layers(l, l, cur)
        torch.cuda.synchronize()
        a, bnp = cur.cpu().numpy(), nxt.cpu().numpy()
        for img in range(2):
            for _ in range(3):
                _check_window(d, param_words[l][0], param_words[l][1], a[img], bnp[img], rng)
        # corners and edges explicitly (true padding)
        for (yy, xx) in [(0, 0), (d.IFM_COL - 24, d.IFM_ROW - 40), (0, d.IFM_ROW - 40)]:
            class _R:  # deterministic "rng" that lands on the requested corner
                def __init__(s, v): s.v = list(v)
                def integers(s, lo, hi): return s.v.pop(0)
            _check_window(d, param_words[l][0], param_words[l][1], a[0], bnp[0], _R([yy // 2, xx // 2]))
        assert int(bnp.max()) <= 127
        sums.append(_sha(bnp))
        cur = nxt
    out, latent = net.forward(_dev(x))
    out1, latent1 = net.forward(_dev(x[1:2]))
    torch.cuda.synchronize()
    assert _sha(out.cpu().numpy()) == sums[7] and _sha(latent.cpu().numpy()) == sums[3]
    assert torch.equal(out[1], out1[0]) and torch.equal(latent[1], latent1[0])


def test_all_64_images_of_the_4k_batch_against_the_oracle_hashes(api):
    """BASELINE.json configs[3] in full on one GPU (VERDICT r4 item 2 i): the job's 64 synthetic 4K images (seeds 0 .. 63) as the 8
    shards an 8-GPU run deals them into — shard r = images r, r + 8, ... (dist.shard_indices) — one after the other through
    EightLayersNet(3840, 2160) with a batch of 8, latent and reconstruction SHA-256 against EVERY entry of
    tests/golden/bench_4k_hashes.json (oracle direct form, tests/golden/make_bench_hashes.py).  Up to round 4 only rank 0's eight
    images had ever met GPU output."""
    from simple_image_compression_network_amd.dist import shard_indices
    golden = json.loads((GOLDEN / "bench_4k_hashes.json").read_text())
    assert all(str(i) in golden for i in range(64))
    net = api.EightLayersNet(3840, 2160)
    out = torch.empty((8,) + net.descs[-1].out_shape, dtype=torch.uint8, device="cuda")
    lat = torch.empty((8,) + net.descs[3].out_shape, dtype=torch.uint8, device="cuda")
    seen = []
    for r in range(8):
        ids = shard_indices(64, r, 8)
        x = np.stack([np.random.default_rng(i).integers(0, 256, (2160, 3840, 3), dtype=np.uint8) for i in ids])
        net.forward(_dev(x), out, lat)
        torch.cuda.synchronize()
        o, l = out.cpu().numpy(), lat.cpu().numpy()
        for k, i in enumerate(ids):
            assert [_sha(l[k]), _sha(o[k])] == golden[str(i)], f"image {i} (shard {r})"
            seen.append(i)
    assert sorted(seen) == list(range(64))


def test_error_codes(api):
    from simple_image_compression_network_amd import _lib
    d = eight_layer_descs(64, 32)[1]
    rng = np.random.default_rng(0)
    _, b, words = _rand_params(rng, d)
    fpw = api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, words)
    x = torch.zeros((1,) + d.in_shape, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.SicnError) as e:          # conv weights handed to the deconv entry point
        api.deconv522(d, fpw, b, x)
    assert e.value.code == -22
    with pytest.raises(TypeError):                    # no CPU path
        api.conv2d(d, fpw, b, x.cpu())
    with pytest.raises(ValueError):
        api.conv2d(replace(d, SIMD=7), fpw, b, x)
    net = api.EightLayersNet(64, 32)
    L = _lib.lib()
    xin = torch.zeros((1, 32, 64, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, 32, 64, 3), dtype=torch.uint8, device="cuda")
    rc = L.sicn_eight_layers_net(net._h, ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), None, 1,
                                 None, 0, None)
    assert rc == -28                                   # SICN_ENOSPC: workspace missing
    assert L.sicn_net_forward(net._h, 3, 1, ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), -1,
                              None, 1, None, 0, None) == -22
    # zero images is a no-op, not an error
    assert L.sicn_eight_layers_net(net._h, ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), None, 0,
                                   None, 0, None) == 0


def test_layer_timing_hooks(api):
    net = api.EightLayersNet(256, 256)
    x = torch.zeros((1, 256, 256, 3), dtype=torch.uint8, device="cuda")
    net.profile(True)
    for _ in range(3):
        net.forward(x)
    ms, cnt = net.layer_ms(reset=True)
    assert cnt == [3] * 8 and all(m > 0 for m in ms)
    ms, cnt = net.layer_ms()
    assert cnt == [0] * 8


def test_cpp_testbench_mirrors_reference_test():
    """tests/cpp/tb_eight_layers_net.cpp = the reference's test_eight_layers_net (conv3_nonsquare_tb.cpp:
    781-1132) over the C++ veneer include/sicn_hls.hpp: all-ones stimulus (reduced size so the naive golden
    model finishes in seconds) and a seeded random image; exit code is the verdict, as in the reference."""
    import subprocess
    from conftest import ROOT
    exe = ROOT / "tests" / "cpp" / "tb_eight_layers_net"
    params = ROOT / "simple_image_compression_network_amd" / "data" / "param_weights.bin"
    assert exe.exists() and params.exists(), "run __graft_entry__.build() first"
    # the last run is the reference's own test at its own size: 768 x 512, all ones (config_nonsquare.h:5-7,
    # conv3_nonsquare_tb.cpp:781-821), golden chain by the oracle's OpenMP direct form
    for args in (["192", "128"], ["96", "80", "7"], ["768", "512", "0", "direct"]):
        r = subprocess.run([str(exe), str(params)] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Image # 0 passed the testing." in r.stdout
        assert "conv2d_layer0: passed" in r.stdout and "deconv2d_layer4: passed" in r.stdout


def test_bench_two_ranks_on_one_gpu_rehearsal():
    """bench.py under torch.distributed.run with 2 ranks (gloo, both on cuda:0): the rank / barrier / MAX-over-ranks /
    rank-0-prints-one-JSON-line logic of the N>1 path, which the driver runs with nccl on a real multi-GPU node."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--backend", "gloo",
           "--width", "256", "--height", "128", "--images-per-gpu", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["global_images"] == 4
    assert d["value"] > 0 and "cpu_baseline" not in d and d["roofline"]["frac"] > 0
    # two distinct shards ran (seeds differ per global image) and both went through the coder round trip
    assert len(d["rank_checksums"]) == 2 and d["rank_checksums"][0] != d["rank_checksums"][1]
    assert d["output_bit_exact"] is None                 # no golden hashes for this rehearsal size
    assert d["with_coder"]["round_trip_exact"] is True and d["with_coder"]["value"] > 0
    # the N > 1 secondaries: strong scaling (64 / N images per rank) and one image over the ranks by bands
    assert d["strong_scaling"]["images_per_gpu"] == 32 and d["strong_scaling"]["value"] > 0
    assert d["banded"]["bands"] == 2 and d["banded"]["equals_one_gpu_bytes"] is True
    assert not [k for k, v in d.items() if isinstance(v, dict) and "error" in v], d     # no secondary leg failed


def test_bench_rccl_code_path_single_rank():
    """The driver runs bench.py with nccl (= RCCL) on N GPUs; a 1-GPU box can at least execute that whole code path — process
    group on the GPU, weight broadcast, barrier, MAX all-reduce of the timed region, checksum all-gather — with one rank
    (SICN_BENCH_FORCE_DIST=1)."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29547", str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
           "--no-hyperprior", "--width", "512", "--height", "256", "--images-per-gpu", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT),
                       env=dict(os.environ, SICN_BENCH_FORCE_DIST="1", SICN_FORCE_COLLECTIVES="1"))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert "nccl" in d["config"]["collectives"] and d["value"] > 0 and d["with_coder"]["round_trip_exact"] is True
    # the N > 1 secondaries ran too, with the band split's all-gather going through RCCL on device tensors (one band here)
    assert d["strong_scaling"]["images_per_gpu"] == 64 and d["strong_scaling"]["value"] > 0
    assert d["banded"]["bands"] == 1 and d["banded"]["equals_one_gpu_bytes"] is True
    assert not [k for k, v in d.items() if isinstance(v, dict) and "error" in v], d


def test_bench_plain_run_dumps_the_timed_outputs(tmp_path):
    """A plain bench.py run prints the headline line and nothing of --full; --dump-outputs writes the timed step's reconstruction and
    latent (whole at this size) as float32, equal to the oracle's for the same seeded images."""
    from conftest import ROOT
    from simple_image_compression_network_amd.config import eight_layer_descs
    W, H, B = 256, 128, 2
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--width", str(W), "--height", str(H),
           "--images-per-gpu", str(B), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert not {"layers", "roofline", "output_bit_exact", "with_coder", "hyperprior", "cpu_baseline", "configs"} & set(d), d
    z = np.load(GOLDEN / "param_weights.npz")
    words, bias = [z[f"w{n}_words"] for n in range(8)], [z[f"b{n}"] for n in range(8)]
    rec, lat = np.load(tmp_path / "reconstruction.npy"), np.load(tmp_path / "latent.npy")
    assert rec.dtype == lat.dtype == np.float32 and rec.shape == (B, H, W, 3)
    for i in range(B):
        x = np.random.default_rng(i).integers(0, 256, (H, W, 3), dtype=np.uint8)
        ref = c_oracle.run_net(eight_layer_descs(W, H), words, bias, x, "direct", threads=4)
        assert np.array_equal(lat[i], ref[3]) and np.array_equal(rec[i], ref[7]), i


def test_committed_small_vectors_on_gpu(api):
    """The HIP path against the committed fixture tests/golden/small_vectors.npz (no oracle call at all)."""
    from test_oracle_golden import _small_vectors
    for d, words, bias, x, y in _small_vectors():
        got = _run_layer(api, d, words, bias, x[None])
        assert np.array_equal(got[0], y), d


def test_reference_compiled_vectors_on_gpu(api):
    """The HIP path against tests/golden/ref_conv_vectors.npz, whose expected outputs were computed by the
    reference's own conv_nonsquare<> (conv.hpp:91-123, compiled unmodified in the build container; see
    tests/golden/make_ref_conv_vectors.py). No oracle call: reference-made bytes vs GPU bytes."""
    from test_oracle_golden import _small_vectors
    n = 0
    for d, words, bias, x, y in _small_vectors("ref_conv_vectors.npz"):
        got = _run_layer(api, d, words, bias, x[None])
        assert np.array_equal(got[0], y), d
        n += 1
    assert n == 10


def test_forward_is_graph_capturable(api):
    """sicn.h promises that launch functions neither allocate nor synchronise: capture the 8-layer chain into a
    hipGraph (torch.cuda.CUDAGraph), replay it on new input and compare with the eager result."""
    net = api.EightLayersNet(256, 256)
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.integers(0, 256, (2, 256, 256, 3), dtype=np.uint8)).cuda()
    out = torch.empty((2, 256, 256, 3), dtype=torch.uint8, device="cuda")
    lat = torch.empty((2, 16, 16, 192), dtype=torch.uint8, device="cuda")
    net.forward(x, out, lat)                      # warm-up outside capture (workspace allocation, module load)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    # nets of earlier tests must not be finalised (hipFree / hipEventDestroy are illegal while a
    # capture is open and would invalidate it) by a garbage collection that happens to run inside
    import gc
    gc.collect()
    torch.cuda.synchronize()
    gc.disable()
    try:
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                net.forward(x, out, lat)
    finally:
        gc.enable()
    x2 = torch.from_numpy(rng.integers(0, 256, (2, 256, 256, 3), dtype=np.uint8)).cuda()
    x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    got_out, got_lat = out.clone(), lat.clone()
    ref_out, ref_lat = net.forward(x2)
    torch.cuda.synchronize()
    assert torch.equal(got_out, ref_out) and torch.equal(got_lat, ref_lat)


def test_capture_helper_replays(api):
    """EightLayersNet.capture: one hipGraph for the 768x512 reference configuration; replay on new input."""
    net = api.EightLayersNet(768, 512)
    x = _dev(_input("ones768")[None])
    out = torch.empty((1, 512, 768, 3), dtype=torch.uint8, device="cuda")
    lat = torch.empty((1, 32, 48, 192), dtype=torch.uint8, device="cuda")
    g = net.capture(x, out, lat)
    x.copy_(_dev(_input("rng768")[None]))
    g.replay()
    torch.cuda.synchronize()
    assert _sha(out[0].cpu().numpy()) == HASHES["layers"]["rng768"][7]
    assert _sha(lat[0].cpu().numpy()) == HASHES["layers"]["rng768"][3]


def test_persistent_kernels_graph_replay_and_two_streams(api):
    """The wide persistent kernels keep no scheduler state (tiles are dealt statically), so a weights handle is immutable:
    (a) a captured forward pass replays correctly any number of times, (b) a graph replaying on one stream while a second
    stream makes 64 eager launches through the SAME sicn_weights disturbs neither (round 2's k_conv_pp
    shared 16 ticket blocks per handle and could not promise this)."""
    opts = {"wave_tile": 128, "persistent_grid": 16}
    net = api.EightLayersNet(768, 512, options=opts)
    x = _dev(np.stack([_input("rng768"), _input("ones768")]))
    out = torch.empty((2, 512, 768, 3), dtype=torch.uint8, device="cuda")
    lat = torch.empty((2, 32, 48, 192), dtype=torch.uint8, device="cuda")
    g = net.capture(x, out, lat)
    for _ in range(5):
        out.zero_()
        g.replay()
    torch.cuda.synchronize()
    for i, name in enumerate(("rng768", "ones768")):
        assert _sha(out[i].cpu().numpy()) == HASHES["layers"][name][7]
        assert _sha(lat[i].cpu().numpy()) == HASHES["layers"][name][3]
    # the graph on one stream, 64 eager forwards through the SAME device weights on another, interleaved
    net2 = api.EightLayersNet(768, 512, options=opts, shared_weights=net.weights)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out2 = torch.empty_like(out)
    torch.cuda.synchronize()
    for it in range(64):
        with torch.cuda.stream(s1):
            if it % 4 == 0:
                out.zero_()
            g.replay()
        with torch.cuda.stream(s2):
            net2.forward(x, out2, want_latent=False, stream=s2)
    torch.cuda.synchronize()
    for o in (out, out2):
        assert _sha(o[0].cpu().numpy()) == HASHES["layers"]["rng768"][7]
        assert _sha(o[1].cpu().numpy()) == HASHES["layers"]["ones768"][7]


def test_banded_single_image_equals_whole_image(api):
    """dist.forward_banded (the optional spatial split): one image cut into horizontal bands with 64 rows of
    recomputed halo, every band through the HIP path on its own, the kept rows put together — byte-identical to one call on
    the whole image (1080 rows: not a multiple of 16; 3 and 5 bands: uneven heights)."""
    from simple_image_compression_network_amd.dist import forward_banded
    w, h = 256, 1080
    img = np.random.default_rng(21).integers(0, 256, (h, w, 3), dtype=np.uint8)
    nets = {}

    def compute(band):
        hb = band.shape[0]
        if hb not in nets:
            nets[hb] = api.EightLayersNet(w, hb)
        out, lat = nets[hb].forward(torch.from_numpy(band[None]).cuda())
        torch.cuda.synchronize()
        return out[0].cpu().numpy(), lat[0].cpu().numpy()

    whole_out, whole_lat = compute(img)
    for n in (3, 5):
        out, lat = forward_banded(compute, img, n_bands=n)
        assert out.shape == whole_out.shape and np.array_equal(out, whole_out), n
        assert np.array_equal(lat, whole_lat), n


def test_randomised_sweep_small():
    """tests/fuzz_parity.py (every kernel family + whole chains on random sizes, strip cuts and tile widths) — a
    short seeded run in a child process; the long runs are manual."""
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "fuzz_parity.py"), "--cases", "60", "--seed", "3", "--chains", "4"],
                       capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "60/60 cases bit-exact" in r.stdout and "4/4 chains bit-exact" in r.stdout


@pytest.mark.parametrize("shape", [(3, 9, 10, 192, 8, 9), (2, 7, 5, 3, 6, 5), (1, 4, 4, 16, 4, 4), (2, 6, 33, 5, 5, 31)])
def test_crop_nhwc_one_launch(api, shape):
    """sicn_crop_nhwc (the hyperprior's scale-map crop): both paths — 16-byte rows and byte rows — against numpy slicing."""
    from simple_image_compression_network_amd import _lib
    n, hs, ws, c, h, w = shape
    src = np.random.default_rng(5).integers(0, 256, (n, hs, ws, c), dtype=np.uint8)
    d_src, d_dst = _dev(src), torch.zeros((n, h, w, c), dtype=torch.uint8, device="cuda")
    rc = _lib.lib().sicn_crop_nhwc(ctypes.c_void_p(d_src.data_ptr()), ctypes.c_void_p(d_dst.data_ptr()), n, hs, ws, h, w, c,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), src[:, :h, :w, :])
    assert _lib.lib().sicn_crop_nhwc(ctypes.c_void_p(d_src.data_ptr()), ctypes.c_void_p(d_dst.data_ptr()), n, hs, ws, hs + 1, w, c, None) == -22
