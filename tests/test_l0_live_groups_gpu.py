"""Layer 0 with three of its four 32-channel groups (k_l0<4, 3>, csrc/k_rgb.hip) and layer 1 behind it, on the copies of its weights
whose K index follows layer 0's permutation (csrc/sicn_live.h, csrc/sicn_abi.hip).  The nets are the first two and three layers of the
reference's net (tests/l0_groups_cases.py): PARAM weights and random ones whose layer-1 input has 48 or 32 dead channels run three
groups; 31 and 0 dead channels are the controls on four.  Behind three groups layer 1, on the wide family here, walks the three planes
that were written (k_conv_g3, tests/test_l1_three_group_walk_gpu.py); plane 3 holds what the workspace held, and a kernel that read it
would meet zero weights there, so the whole workspace is filled with seeded random bytes before every call and two different fills must
give the same bytes.
Geometries (input W x H of layer 0): 2 x 2 and 14 x 10 (less than a tile, less than a strip); 260 x 136 x 3 (layer 0 writes 130 x 68:
five strips, the last 2 wide, 9 tiles high; layer 1 writes 65 x 34 = 3 x 3 ragged tiles, a workgroup walking tiles across image
boundaries) and 400 x 180 x 3 (layer 1: 4 x 3 tiles, 4 - 5 per workgroup) on 8 / 16 / all workgroups; 260 x 136 x 3 on the smallest
grid (one workgroup per XCD at most); and the dynamic tile deal with the images sized from the chip: three calls, one in a workspace
without deal words, one captured graph replayed twice.  strip_chunks 1 / 2 / 3 cut layer 0's runs; a tap at layer 1 runs it with all 8
columns over the garbage plane; the full PARAM net on 132 x 68 is held to the oracle, latent and reconstruction.
Every case first asserts what ran (sicn_debug_net_groups, sicn_debug_net_columns, the families of sicn_debug_plan), then compares every
byte of the last layer with the C oracle's direct form."""
import ctypes

import numpy as np
import pytest

import l0_groups_cases as gc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KK_MFMA_CONV, KK_L0_RGB = 1, 3               # csrc/sicn_internal.h KernelKind = out[2] of sicn_debug_plan

# input W x H of layer 0, images (0: sized from the chip), grids, dealt dynamically
ROWS = [
    (2, 2, 3, (8,), False),
    (14, 10, 3, (8,), False),
    (260, 136, 3, (8, 16, 0, 1), False),
    (400, 180, 3, (8, 16, 0), False),
    (260, 136, 0, (8,), True),
]


def _cases():
    return [pytest.param(w, h, n, grid, deal, id=f"{w}x{h}-grid{grid}" + ("-deal" if deal else ""))
            for w, h, n, grids, deal in ROWS for grid in grids]


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
    """seeded random bytes in the whole workspace: the ping-pong buffers (plane 3 of layer 0's output among them) and the deal words"""
    ws = net.workspace(n)
    ws.copy_(torch.from_numpy(np.random.default_rng(seed).integers(0, 256, ws.numel(), dtype=np.uint8)))
    torch.cuda.synchronize()


def _build(api, wset, w, h, n, n_layers, grid, deal=False, tap=-1, **options):
    """the net, with everything that says what a call of it runs asserted; returns (net, input on the device, references per layer)"""
    descs = gc.descs(w, h, n_layers)
    params = [(api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, gc.words(l, gc.weights(wset, l)[0])), gc.weights(wset, l)[1])
              for l, d in enumerate(descs)]
    options = dict({"wave_tile": 128, "persistent_grid": grid}, **options)
    net = api.EightLayersNet(descs=descs, params=params, options=options)
    last = n_layers - 1
    g = gc.groups(wset)
    g_out, g_in = _net_ints("sicn_debug_net_groups", net, last, tap, n)
    assert g_out == [g] + [4] * last and g_in == [4, g] + [4] * (last - 1), (g_out, g_in)
    cols, live = _net_ints("sicn_debug_net_columns", net, last, tap, n)
    l1_cols = 5 if (n_layers == 3 and tap != 1) else 8
    assert cols == [8, l1_cols, 8][:n_layers], cols
    assert live[0] == 128 - gc.SETS[wset] and live[1] == (128 - gc.L2_DEAD if l1_cols == 5 else 128), live
    n_cu, n_xcd = _chip()
    assert _plan(descs[0], n, n_cu, **options)[2] == KK_L0_RGB
    for d in descs[1:]:                          # the wide persistent family, dealt as the row says
        plan = _plan(d, n, n_cu, **options)
        assert plan[2] == KK_MFMA_CONV and plan[3] == 2, plan
    plan = _plan(descs[1], n, n_cu, **options)
    assert plan[10] == int(deal), plan
    if deal:
        assert plan[7] == max(grid // n_xcd * n_xcd, n_xcd), plan
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
def test_first_layers_are_the_oracles(api, w, h, n, grid, deal, wset, n_layers):
    if deal:
        n = _deal_images(w, h, grid)
    net, xin, refs = _build(api, wset, w, h, n, n_layers, grid, deal)
    last = n_layers - 1
    what = f"{wset} {w}x{h} x {n}, layers 0 .. {last}, grid {grid}"
    out = None
    for call in range(3 if deal else 2):         # two different fills of the workspace: the same bytes
        _garbage(net, n, 100 + call)
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
    _garbage(net, n, 150)
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
        _garbage(net, n, 200 + replay)
        g.replay()
        torch.cuda.synchronize()
        _same(out, refs[last], f"{what}, graph replay {replay}")


@pytest.mark.parametrize("chunks", [1, 2, 3])
@pytest.mark.parametrize("wset", ["param", "r32", "r31"])
def test_layer_0_runs_cut_by_strip_chunks(api, wset, chunks):
    """130 x 68 outputs: 9 tiles per strip in one run of 9, in 5 + 4 and in 3 + 3 + 3"""
    w, h, n = 260, 136, 3
    net, xin, refs = _build(api, wset, w, h, n, 2, 8, strip_chunks=chunks)
    n_cu, _ = _chip()
    plan = _plan(net.descs[0], n, n_cu, wave_tile=128, persistent_grid=8, strip_chunks=chunks)
    assert plan[7:12] == [5, chunks, n, chunks, (9 + chunks - 1) // chunks], plan
    _garbage(net, n, 300 + chunks)
    out, _ = net.run_layers(0, 1, xin)
    torch.cuda.synchronize()
    _same(out, refs[1], f"{wset} 260x136, strip_chunks {chunks}")


@pytest.mark.parametrize("wset", ["param", "r48", "r32", "r31"])
def test_tap_at_layer_1_keeps_its_columns_over_the_garbage_plane(api, wset):
    """layer 0 has three groups, layer 1 (tapped: all 8 columns, the input-permuted copy) walks four planes, layer 2 reads the tap"""
    w, h, n = 260, 136, 3
    net, xin, refs = _build(api, wset, w, h, n, 3, 8, tap=1)
    for call in range(2):
        _garbage(net, n, 400 + call)
        out, tap = net.run_layers(0, 2, xin, tap_layer=1)
        torch.cuda.synchronize()
        _same(tap, refs[1], f"{wset}: the tap at layer 1, call {call}")
        _same(out, refs[2], f"{wset}: layer 2 behind the tap, call {call}")


def test_tap_at_layer_0_and_a_call_that_ends_there_keep_four_groups(api):
    w, h, n = 260, 136, 3
    net, xin, refs = _build(api, "param", w, h, n, 3, 8)
    for last, tap in ((0, -1), (2, 0)):
        g_out, g_in = _net_ints("sicn_debug_net_groups", net, last, tap, n)
        assert g_out == [4, 4, 4] and g_in == [4, 4, 4], (g_out, g_in)
        _garbage(net, n, 500 + last)
        out, t = net.run_layers(0, last, xin, tap_layer=tap)
        torch.cuda.synchronize()
        _same(out, refs[last], f"call [0, {last}], tap {tap}")
        if tap == 0:
            _same(t, refs[0], "the tap at layer 0: every channel, in its own order")


def test_full_param_net_latent_and_reconstruction(api):
    """the 8-layer PARAM net on 132 x 68: layer 0 with three groups in front of the live-column kernels and the one-half layer 7"""
    from oracle import sicn_ref
    w, h, n = 132, 68, 3
    options = {"wave_tile": 128, "persistent_grid": 8}
    net = api.EightLayersNet(w, h, options=options)
    g_out, g_in = _net_ints("sicn_debug_net_groups", net, 7, 3, n)
    assert g_out == [3] + [4] * 7 and g_in == [4, 3] + [4] * 6, (g_out, g_in)
    cols, _ = _net_ints("sicn_debug_net_columns", net, 7, 3, n)
    assert cols == [8, 5, 5, 8, 8, 5, 3, 8], cols
    x = np.random.default_rng([gc.SEED, 9]).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    params = sicn_ref.load_param_fixture(gc.GOLDEN)
    refs = [sicn_ref.eight_layers_net_ref(x[i], params) for i in range(n)]
    xin = torch.from_numpy(x).cuda()
    for call in range(2):
        _garbage(net, n, 600 + call)
        out, latent = net.forward(xin)
        torch.cuda.synchronize()
        _same(latent, [r[3] for r in refs], f"latent, call {call}")
        _same(out, [r[7] for r in refs], f"reconstruction, call {call}")
