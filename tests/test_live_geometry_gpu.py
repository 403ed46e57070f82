"""The live-column kernels (k_conv_live / k_deconv_live<NT, 3 | 5>, csrc/k_mfma16x_live.hip) and the one-half layer 7 (k_l7<1>,
csrc/k_rgb.hip) at the edges of their geometry.  tests/test_live_columns_gpu.py and tests/test_l7_live_half_gpu.py run them inside
8-layer nets on 132 x 68: one or four tiles per image, at most two tiles per workgroup, even deconv maps only, layer 7 on whole steps,
and (random weights) 16 of the 48 channels of a 3-column kernel read by anybody.  Here a two- or three-layer net of custom descriptors
(tests/live_geometry_cases.py) puts the producer, conv or deconv 128 -> 128, on the geometries that tests/test_gpu_parity.py holds the
8-column kernels to: 1 x 1, sub-tile, ragged tile maps with a workgroup walking 3 .. 5 tiles across image boundaries, 8 / 16 / all
workgroups, odd deconv maps, and the smallest map that the dynamic tile deal accepts (>= 16 tiles per workgroup: three calls, one
more in a workspace of the old size, which deals the same tiles statically, and a replayed graph).  The consumer's weights make 80 / 48 / 0 of the producer's channels dead: 3 columns with all 48 computed positions
read, 5 with all 80, and the 8-column control that tells a fault of this file from a fault of a live kernel.
Behind the deconv producer sits layer 7 (deconv 128 -> 3): behind 3 columns it reads one half.  At 33 x 17 it sees 66 x 34: three
strips, the last one 2 columns wide, and 9 steps of 4 rows, the last one 2 rows; strip_chunks = 1 is one run of 9 steps through a ring
that wraps, 2 is 5 + 4 and 3 is 3 + 3 + 3.
Every case first asserts what ran (columns, live outputs, halves, family and deal flag of the plan), then compares every byte with the C
oracle's direct form, layer by layer; the workspace is filled with seeded random bytes before every call, so a position that nobody
computed holds garbage, not zeros."""
import ctypes

import numpy as np
import pytest

import live_geometry_cases as lg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 20

# producer, input W x H of the producer, images, grids, dealt dynamically
ROWS = [
    ("conv", 1, 1, 3, (8,), False),                # one position; 3 tiles on 8 workgroups: 5 of them return at once
    ("conv", 7, 5, 3, (8,), False),                # 4 x 3 positions: less than a tile
    ("conv", 129, 67, 3, (8, 16, 0), False),       # 65 x 34 = 3 x 3 tiles, last column 1 wide, last row 2 high; up to 4 tiles per workgroup
    ("conv", 200, 90, 3, (8, 16, 0), False),       # 100 x 45 = 4 x 3 tiles; 4 - 5 tiles per workgroup
    ("conv", 250, 104, 0, (8,), True),             # 125 x 52 = 4 x 4 tiles, ragged at both edges; images sized from the chip (below)
    ("deconv", 1, 1, 3, (8,), False),
    ("deconv", 7, 5, 3, (8,), False),              # layer 7 sees 14 x 10: one strip narrower than 32
    ("deconv", 33, 17, 3, (8,), False),            # 2 x 2 tiles, 1 column / 1 row over; layer 7 sees 66 x 34
    ("deconv", 65, 19, 3, (8, 16, 0), False),      # 3 x 2 tiles, odd map
    ("deconv", 100, 45, 3, (8, 16, 0), False),     # 4 x 3 tiles
    ("deconv", 125, 52, 0, (8,), True),            # 4 x 4 tiles, the dynamic deal
]
DECONV_TWICE = {(65, 19), (100, 45)}               # the deconv geometries that also run a deconv 128 -> 128 as the consumer


def _cases():
    out = []
    for prod, w, h, n, grids, deal in ROWS:
        consumers = ["conv"] if prod == "conv" else ["rgb"] + (["deconv"] if (w, h) in DECONV_TWICE else [])
        for cons in consumers:
            for grid in grids:
                out.append(pytest.param((prod, cons), w, h, n, grid, deal, id=f"{prod}{w}x{h}-{cons}-grid{grid}"))
    return out


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import api as _api
    return _api


def _chip():
    from simple_image_compression_network_amd import _lib
    chip = (ctypes.c_int32 * 2)()
    _lib.check(_lib.lib().sicn_debug_chip(chip), "sicn_debug_chip")
    return int(chip[0]), int(chip[1])


def _plan(d, n, n_cu, **options):
    from simple_image_compression_network_amd import _lib
    plan = (ctypes.c_int32 * 12)()
    _lib.check(_lib.lib().sicn_debug_plan(ctypes.byref(d.to_c()), n, ctypes.byref(_lib.make_options(**options)), n_cu, plan), "sicn_debug_plan")
    return list(plan)


def _net_ints(fn, net, n, *arrays):
    from simple_image_compression_network_amd import _lib
    _lib.check(getattr(_lib.lib(), fn)(net._h, 0, len(net.descs) - 1, -1, n, *arrays), fn)
    return [list(a)[:len(net.descs)] for a in arrays]


def _same(got, want, what):
    got = got.cpu().numpy()
    for i in range(len(want)):
        if not np.array_equal(got[i], want[i]):
            bad = np.argwhere(got[i] != want[i])
            y, xx, c = (int(v) for v in bad[0])
            raise AssertionError(f"{what}, image {i}: {len(bad)} wrong bytes in channels {sorted({int(v) for v in bad[:, 2]})[:16]}, rows "
                                 f"{sorted({int(v) for v in bad[:, 0]})[:12]}, columns {sorted({int(v) for v in bad[:, 1]})[:12]}; "
                                 f"first: got {got[i][y, xx, c]} want {want[i][y, xx, c]} at ({y}, {xx}, {c})")


def _garbage(net, n, seed):
    """seeded random bytes in the whole workspace: the ping-pong buffers and the deal words (which every call zeroes itself)"""
    ws = net.workspace(n)
    ws.copy_(torch.from_numpy(np.random.default_rng(seed).integers(0, 256, ws.numel(), dtype=np.uint8)))
    torch.cuda.synchronize()


def _build(api, kinds, w, h, n, grid, cols, deal, **options):
    """the net, with everything that says what a call of it runs asserted; returns (net, input on the device, reference of the last layer)"""
    n_dead = lg.N_DEAD[cols]
    descs = lg.chain_descs(kinds, w, h)
    params = [(api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, lg.words(k, wt)), b)
              for k, d, (wt, b) in zip(kinds, descs, lg.chain_weights(kinds, SEED, n_dead))]
    options = dict({"wave_tile": 128, "persistent_grid": grid}, **options)
    net = api.EightLayersNet(descs=descs, params=params, options=options)
    last = len(kinds) - 1
    c, live = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)()
    c, live = _net_ints("sicn_debug_net_columns", net, n, c, live)
    assert c == [cols] * last + [8] and live[:last] == [128 - n_dead] * last, (c, live)
    halves, = _net_ints("sicn_debug_net_input_halves", net, n, (ctypes.c_int32 * 8)())
    assert halves == [2] * last + [1 if kinds[-1] == "rgb" and cols == 3 else 2], halves
    n_cu, n_xcd = _chip()
    for d in descs[:last]:                       # the layers that skip columns: the wide family, dealt as the row says
        plan = _plan(d, n, n_cu, **options)
        assert plan[3] == 2 and plan[10] == int(deal), plan
        if deal:
            assert plan[7] == max(grid // n_xcd * n_xcd, n_xcd), plan
    ref = lg.reference(kinds, w, h, n, SEED, n_dead)[-1]
    return net, torch.from_numpy(lg.images(SEED, descs[0], n)).cuda(), ref


def _deal_images(kinds, w, h, grid):
    """the fewest images with which every workgroup walks >= 16 tiles (csrc/sicn_plan.h wide_deal_pays), on the grid this chip leaves"""
    n_xcd = _chip()[1]
    tx, ty = lg.tiles(lg.desc(kinds[0], w, h))
    return (16 * max(grid // n_xcd * n_xcd, n_xcd) + tx * ty - 1) // (tx * ty)


@pytest.mark.parametrize("cols", [3, 5, 8])
@pytest.mark.parametrize("kinds, w, h, n, grid, deal", _cases())
def test_two_layers_are_the_oracles(api, kinds, w, h, n, grid, deal, cols):
    if deal:
        n = _deal_images(kinds, w, h, grid)
    net, xin, ref = _build(api, kinds, w, h, n, grid, cols, deal)
    what = f"{kinds[0]} {w}x{h} x {n} -> {kinds[1]}, grid {grid}, {cols} columns"
    out = None
    for call in range(3 if deal else 1):
        _garbage(net, n, 100 + call)
        out, _ = net.run_layers(0, 1, xin)
        torch.cuda.synchronize()
        _same(out, ref, f"{what}, call {call}")
    if not deal:
        return
    # a workspace of the old size, without room for the deal words (include/sicn.h): the same 16 tiles per workgroup, all dealt statically
    L = api._lib.lib()
    full = int(L.sicn_net_workspace_bytes(net._h, n))
    small = full - (len(kinds) * 528 * 8 + 255) // 256 * 256          # the deal words of every layer, as csrc/sicn_abi.hip aligns them
    assert 0 < small < full
    _garbage(net, n, 150)
    static = torch.zeros_like(out)
    rc = L.sicn_net_forward(net._h, 0, 1, ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(static.data_ptr()), -1, None, n,
                            ctypes.c_void_p(net.workspace(n).data_ptr()), small, api._stream_ptr(None))
    torch.cuda.synchronize()
    assert rc == 0, rc
    _same(static, ref, f"{what}, static deal in a workspace of {small} of {full} bytes")
    # the deal words are zeroed by every call; in a captured graph the zeroing is a node
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            net.run_layers(0, 1, xin, out=out)
    for replay in range(2):
        out.zero_()
        _garbage(net, n, 200 + replay)
        g.replay()
        torch.cuda.synchronize()
        _same(out, ref, f"{what}, graph replay {replay}")


@pytest.mark.parametrize("chunks", [0, 1, 2, 3])
@pytest.mark.parametrize("cols", [3, 5])
def test_layer_7_partial_step_narrow_strip_and_ring_wrap(api, cols, chunks):
    """layer 7 on 66 x 34 (the module's docstring), one half behind 3 columns and both behind 5, in 9 / 1 / 2 / 3 runs per strip"""
    kinds, w, h, n = ("deconv", "rgb"), 33, 17, 3
    net, xin, ref = _build(api, kinds, w, h, n, 8, cols, False, strip_chunks=chunks)
    n_cu, _ = _chip()
    plan = _plan(net.descs[1], n, n_cu, wave_tile=128, persistent_grid=8, strip_chunks=chunks)
    assert (net.descs[1].IFM_ROW, net.descs[1].IFM_COL) == (66, 34)
    assert plan[2] == 4 and plan[10] == (chunks or min(9, max(1, 2 * n_cu // (3 * n)))), plan      # csrc/sicn_plan.h plan_l7
    _garbage(net, n, 300 + chunks)
    out, _ = net.run_layers(0, 1, xin)
    torch.cuda.synchronize()
    _same(out, ref, f"deconv 33x17 -> layer 7, {cols} columns, strip_chunks {chunks}")


@pytest.mark.parametrize("kinds, w, h", [(("conv", "conv", "conv192"), 129, 67), (("deconv", "deconv", "rgb"), 33, 17)],
                         ids=["conv129x67-conv-conv192", "deconv33x17-deconv-rgb"])
def test_three_layers_middle_one_permuted_on_both_sides(api, kinds, w, h):
    """80 dead channels in both consumers: the middle layer reads permuted channels, runs 3 columns itself and writes permuted channels"""
    n = 3
    net, xin, ref = _build(api, kinds, w, h, n, 8, 3, False)
    _garbage(net, n, 400)
    out, _ = net.run_layers(0, 2, xin)
    torch.cuda.synchronize()
    _same(out, ref, " -> ".join(kinds) + f" {w}x{h}")
