"""Layer 1 behind a layer 0 that stored three of its four 32-channel groups: the wide conv walks K over the three groups that exist
(k_conv_g3, csrc/k_mfma16x_g3.hip; the schedule: csrc/conv_walk.hpp) — a tile of 40 passes, the next tile's first group requested in
the tile's last ten.  The nets, weight sets, images and oracle outputs are tests/l0_groups_cases.py's (shared with
tests/test_l0_live_groups_gpu.py, whose docstring still says "four planes" of this layer: that was the kernel before this one): PARAM
and random weights with 48 or 32 dead layer-1 inputs run three groups (80 live: group 2 half full; 96: full), 31 and 0 dead are the
controls on the four-group kernels.
Geometries (input W x H of layer 0), the smallest at which the walk can still go wrong: 14 x 10 x 1 (one sub-tile: the prologue, one tile
and the final hand-over with no next tile); 260 x 136 x 3 on 8 workgroups (layer 1 writes 65 x 34 = 3 x 3 ragged tiles, a workgroup
walks 3 - 4 of them across image boundaries: the next-tile requests of the tile's second window cross the tile and image switch) and on
one workgroup per XCD (the longest chain of tiles); 260 x 136 with the images sized from the chip (the dynamic deal: one call in a
workspace without deal words, one captured graph replayed twice).  Three layers: layer 1 has 5 columns; two: it is the call's last and
has 8; a tap at layer 1: 8 columns in the middle of a chain.
Every case first asserts what ran — sicn_debug_net_walk_groups, sicn_debug_net_groups and sicn_debug_net_columns (fields of the call plan that sicn_net_forward executes:
live::plan_call, csrc/sicn_live.h), the families of sicn_debug_plan — then compares every byte with the C oracle's direct
form, with the whole workspace filled with two different seeded garbage patterns."""
import ctypes

import numpy as np
import pytest

import l0_groups_cases as gc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KK_MFMA_CONV, KK_L0_RGB = 1, 3               # csrc/sicn_internal.h KernelKind = out[2] of sicn_debug_plan

# input W x H of layer 0, images (0: sized from the chip), grid (1: one workgroup per XCD), dealt dynamically
ROWS = [
    (14, 10, 1, 8, False),
    (260, 136, 3, 8, False),
    (260, 136, 3, 1, False),
    (260, 136, 0, 8, True),
]


def _cases():
    return [pytest.param(w, h, n, grid, deal, id=f"{w}x{h}-grid{grid}" + ("-deal" if deal else "")) for w, h, n, grid, deal in ROWS]


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


def _net_ints(fn, net, last, tap, n, count=2):
    from simple_image_compression_network_amd import _lib
    arrays = [(ctypes.c_int32 * 8)() for _ in range(count)]
    _lib.check(getattr(_lib.lib(), fn)(net._h, 0, last, tap, n, *arrays), fn)
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
    """seeded random bytes in the whole workspace: the ping-pong buffers (the plane layer 0 does not write among them) and the deal words"""
    ws = net.workspace(n)
    ws.copy_(torch.from_numpy(np.random.default_rng(seed).integers(0, 256, ws.numel(), dtype=np.uint8)))
    torch.cuda.synchronize()


def _make(api, layer_weights, w, h, n, grid, groups, l1_cols, n_live1, tap=-1, deal=False):
    """the net of layer_weights = [(W, bias)], with everything that says what a call of it runs asserted"""
    n_layers = len(layer_weights)
    descs = gc.descs(w, h, n_layers)
    params = [(api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, gc.words(l, layer_weights[l][0])), layer_weights[l][1])
              for l, d in enumerate(descs)]
    options = {"wave_tile": 128, "persistent_grid": grid}
    net = api.EightLayersNet(descs=descs, params=params, options=options)
    last = n_layers - 1
    n_cu, n_xcd = _chip()
    assert _plan(descs[0], n, n_cu, **options)[2] == KK_L0_RGB
    for d in descs[1:]:                          # the wide persistent family
        plan = _plan(d, n, n_cu, **options)
        assert plan[2] == KK_MFMA_CONV and plan[3] == 2, plan
    plan = _plan(descs[1], n, n_cu, **options)
    assert plan[10] == int(deal), plan
    if deal:
        assert plan[7] == max(grid // n_xcd * n_xcd, n_xcd), plan
    (walk,) = _net_ints("sicn_debug_net_walk_groups", net, last, tap, n, count=1)
    assert walk == [4, groups] + [4] * (last - 1), walk            # layer 1 walks what layer 0 stored, nobody else changes
    g_out, g_in = _net_ints("sicn_debug_net_groups", net, last, tap, n)
    assert g_out == [groups] + [4] * last and g_in == [4, groups] + [4] * (last - 1), (g_out, g_in)
    cols, live = _net_ints("sicn_debug_net_columns", net, last, tap, n)
    assert cols == [8, l1_cols, 8][:n_layers], cols
    assert live[0] == n_live1, live
    return net


def _build(api, wset, w, h, n, n_layers, grid, deal=False, tap=-1):
    weights = [gc.weights(wset, l) for l in range(n_layers)]
    l1_cols = 5 if (n_layers == 3 and tap != 1) else 8
    net = _make(api, weights, w, h, n, grid, gc.groups(wset), l1_cols, 128 - gc.SETS[wset], tap, deal)
    return net, torch.from_numpy(gc.images(w, h, n)).cuda(), gc.reference(wset, w, h, n, n_layers)


def _deal_images(w, h, grid):
    """the fewest images with which every workgroup of layer 1 walks >= 16 tiles (csrc/sicn_plan.h wide_deal_pays), on this chip's grid"""
    n_xcd = _chip()[1]
    d = gc.descs(w, h, 2)[1]
    tiles = ((d.OFM_ROW + 31) // 32) * ((d.OFM_COL + 15) // 16)
    return (16 * max(grid // n_xcd * n_xcd, n_xcd) + tiles - 1) // tiles


@pytest.mark.parametrize("n_layers", [2, 3])
@pytest.mark.parametrize("wset", list(gc.SETS))
@pytest.mark.parametrize("w, h, n, grid, deal", _cases())
def test_layer_1_behind_three_groups_is_the_oracles(api, w, h, n, grid, deal, wset, n_layers):
    if deal:
        n = _deal_images(w, h, grid)
    net, xin, refs = _build(api, wset, w, h, n, n_layers, grid, deal)
    last = n_layers - 1
    what = f"{wset} {w}x{h} x {n}, layers 0 .. {last}, grid {grid}"
    out = None
    for call in range(2):                        # two different fills of the workspace: the same bytes
        _garbage(net, n, 700 + call)
        out, _ = net.run_layers(0, last, xin)
        torch.cuda.synchronize()
        _same(out, refs[last], f"{what}, call {call}")
    if not deal:
        return
    # a workspace without room for the deal words (include/sicn.h): the same tiles, dealt statically
    L = api._lib.lib()
    full = int(L.sicn_net_workspace_bytes(net._h, n))
    small = full - (n_layers * 528 * 8 + 255) // 256 * 256          # the deal words of every layer, as csrc/sicn_abi.hip aligns them
    assert 0 < small < full
    _garbage(net, n, 750)
    static = torch.zeros_like(out)
    rc = L.sicn_net_forward(net._h, 0, last, ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(static.data_ptr()), -1, None, n,
                            ctypes.c_void_p(net.workspace(n).data_ptr()), small, api._stream_ptr(None))
    torch.cuda.synchronize()
    assert rc == 0, rc
    _same(static, refs[last], f"{what}, static deal in a workspace of {small} of {full} bytes")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            net.run_layers(0, last, xin, out=out)
    for replay in range(2):
        out.zero_()
        _garbage(net, n, 800 + replay)
        g.replay()
        torch.cuda.synchronize()
        _same(out, refs[last], f"{what}, graph replay {replay}")


@pytest.mark.parametrize("wset", list(gc.SETS))
@pytest.mark.parametrize("w, h, n, grid", [(14, 10, 1, 8), (260, 136, 3, 8), (260, 136, 3, 1)])
def test_tap_at_layer_1_walks_three_groups_with_all_columns(api, w, h, n, grid, wset):
    """layer 1 is tapped: all 8 columns in the middle of a chain, on the input-permuted copy alone; layer 2 reads the tap"""
    net, xin, refs = _build(api, wset, w, h, n, 3, grid, tap=1)
    for call in range(2):
        _garbage(net, n, 900 + call)
        out, tap = net.run_layers(0, 2, xin, tap_layer=1)
        torch.cuda.synchronize()
        _same(tap, refs[1], f"{wset} {w}x{h} grid {grid}: the tap at layer 1, call {call}")
        _same(out, refs[2], f"{wset} {w}x{h} grid {grid}: layer 2 behind the tap, call {call}")


def _k_order_weights(n_live):
    """Layer 1 for the K order: 128 - n_live random dead input channels; in the output channels 0 .. 126 the only non-zero weights sit on
    tap (3, 3) — the last of the plane-ordered walk — of the LAST live channel (position n_live - 1 behind layer 0's permutation: with 96
    live channels the last byte of stream step 74, the last real K step) and on tap (0, 0) of the FIRST live channel (position 0: the
    first byte of step 0), every value distinct from its neighbour's.  A weight stream that is one step off at the 75 / 80 seam or at
    the wrap loses one of the two products, or multiplies it with a neighbouring tap's pixels.  Output channel 127 alone has a weight on
    every live channel (tap (2, 2)): that is what keeps n_live channels live, and so the last one at position n_live - 1."""
    rng = np.random.default_rng([gc.SEED, 4242, n_live])
    alive = np.sort(rng.permutation(128)[:n_live])
    w = np.zeros((128, 5, 5, 128), np.int8)
    o = np.arange(127)
    w[o, 3, 3, alive[-1]] = (o % 7 + 1).astype(np.int8)              # 1 .. 7
    w[o, 0, 0, alive[0]] = -((o + 3) % 8 + 1).astype(np.int8)        # -1 .. -8
    w[127, 2, 2, alive] = 1
    b = rng.integers(-128, 128, 128).astype(np.int8)
    return w, b


@pytest.mark.parametrize("n_layers", [2, 3])
@pytest.mark.parametrize("n_live", [96, 80])
def test_k_order_at_the_seam_and_the_wrap(api, n_live, n_layers):
    w, h, n, grid = 260, 136, 3, 8
    weights = [gc.weights("r0", 0), _k_order_weights(n_live)] + ([gc.weights("r0", 2)] if n_layers == 3 else [])
    net = _make(api, weights, w, h, n, grid, 3, 5 if n_layers == 3 else 8, n_live)
    x = gc.images(w, h, n)
    refs = gc.reference("r0", w, h, n, 1)                            # layer 0 of every random set is the same layer
    for l in range(1, n_layers):
        refs.append(gc.oracle_layer(l, net.descs[l], weights[l], refs[-1]))
    assert len(np.unique(refs[1][..., :127])) > 8, "the two products reach the output"
    xin = torch.from_numpy(x).cuda()
    for call in range(2):
        _garbage(net, n, 1000 + call)
        out, _ = net.run_layers(0, n_layers - 1, xin)
        torch.cuda.synchronize()
        _same(out, refs[-1], f"K order, {n_live} live, layers 0 .. {n_layers - 1}, call {call}")
