"""The size limits of include/sicn.h, run: one image just under 2 GiB through every kernel family (A), the first refused size of each
(B), batches whose image bases lie on both sides of 2^32 (C), sicn_gdn_apply over more than one chunk of lanes (E) and the
non-temporal stores of the wide and live-column kernels at the smallest launch that selects them (F).  tests/large_tensor_cases.py
holds the shapes and the checker, tests/test_large_tensors.py holds both to arithmetic and to the oracle.
A result of this size is checked twice.  Windows: crops of at most 40 x 24 input pixels, read from the device by slicing, go through
the C oracle's direct form and are compared where their receptive field lies inside the crop or at a true edge: the four corners (the
last one holds the tensor's last byte), the byte offsets 2^28, 2^29 and 2^30 of the output, the last rows, and six seeded ones.  Bands:
the input is cut into 16 horizontal bands, each band runs through the same layers as a small image of its own (tensors under 160 MB: the
offsets and plans that the rest of the suite holds to the oracle; normally another kernel family, never non-temporal stores), and every
row of the big result is compared on the device with the band that holds its receptive field.
Every tensor is drawn on the device from a seeded generator, weights are random nibbles with a bias per channel.  Before a call the
case asserts what will run (sicn_debug_plan, sicn_debug_net_columns / _input_halves / _groups), so a case that falls to another
kernel fails.  Every output lies between guard bands of 4 KiB and is filled with a byte that no layer writes.  A test frees what it
allocated; none holds more than 8 GiB, except the one refused call noted at test_rgb_batch_limit.
D: one-layer ragged nets, the packed RGB ends among them, and RaggedCrop / RaggedCut over a 128-channel tensor of 4.3 GB in which an
image straddles 2^32 and two begin beyond it.
Left out: the accepted side of the RGB batch limit (86 images of 3840 x 2160 need an output of 22.8 GB)."""
import ctypes

import numpy as np
import pytest

import large_tensor_cases as lt
import live_geometry_cases as lg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 41
N_BANDS = 16
FILL, EDGE = 0xC3, 0x5A                     # no layer writes 0xC3 behind a ReLU (outputs are 0 .. 127); the guard bands hold 0x5A
EINVAL = -22


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import api as _api
    return _api


@pytest.fixture(autouse=True)
def _free():
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _lib():
    from simple_image_compression_network_amd import _lib as m
    return m


def _chip():
    chip = (ctypes.c_int32 * 2)()
    _lib().check(_lib().lib().sicn_debug_chip(chip), "sicn_debug_chip")
    return int(chip[0]), int(chip[1])


def _plan(d, n, **options):
    plan = (ctypes.c_int32 * 12)()
    _lib().check(_lib().lib().sicn_debug_plan(ctypes.byref(d.to_c()), n, ctypes.byref(_lib().make_options(**options)), _chip()[0], plan),
                 "sicn_debug_plan")
    return list(plan)


def _net_ints(fn, net, n, *arrays):
    _lib().check(getattr(_lib().lib(), fn)(net._h, 0, len(net.descs) - 1, -1, n, *arrays), fn)
    return [list(a)[:len(net.descs)] for a in arrays]


def _random(shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)


def _guarded(shape, fill=FILL):
    """(buffer, view of `shape` between two guard bands)"""
    nbytes = int(np.prod(shape, dtype=np.int64))
    buf = torch.full((nbytes + 2 * lt.GUARD,), fill, dtype=torch.uint8, device="cuda")
    buf[:lt.GUARD] = EDGE
    buf[lt.GUARD + nbytes:] = EDGE
    return buf, buf[lt.GUARD:lt.GUARD + nbytes].view(shape)


def _guards_intact(buf):
    return bool((buf[:lt.GUARD] == EDGE).all()) and bool((buf[-lt.GUARD:] == EDGE).all())


def _all_bytes_are(t, value):
    """a tensor of gigabytes against one byte without a temporary of its size"""
    flat = t.reshape(-1)
    n8 = flat.numel() // 8 * 8
    word = int.from_bytes(bytes([value]) * 8, "little", signed=True)
    return bool((flat[:n8].view(torch.int64) == word).all()) and bool((flat[n8:] == value).all())


def _device_weights(api, kinds, wb, w=8, h=8):
    """one DeviceWeights per layer (they do not depend on the image size)"""
    return [api.DeviceWeights(d, api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, lt.words(k, wt)), b)
            for k, d, (wt, b) in zip(kinds, lt.chain_descs(kinds, w, h), wb)]


def _layer(api, kind, dw, x, w, h, out=None, options=None):
    """one layer on x [n][h][w][c] through the per-layer entry point"""
    d = lt.desc(kind, w, h)
    fn = api.deconv522 if d.transposed else api.conv2d
    return fn(d, dw, None, x, out, numReps=x.shape[0], options=options)


def _windows(kinds, wb, x, out, w, h, what, gdn=None, last_rows=False):
    """x [h][w][c] and out [oh][ow][c] on the device, one image"""
    for oy, ox in lt.window_positions(kinds, w, h, SEED, last_rows=last_rows):
        y0, y1, ylo, yhi, yoff = lt.window(kinds, h, oy, lt.WINDOW_H)
        x0, x1, xlo, xhi, xoff = lt.window(kinds, w, ox, lt.WINDOW_W)
        ref = lt.oracle_chain(kinds, wb, x[y0:y1, x0:x1].cpu().numpy(), gdn)[ylo:yhi, xlo:xhi]
        got = out[yoff + ylo:yoff + yhi, xoff + xlo:xoff + xhi].cpu().numpy()
        bad = lt.first_difference(got, ref)
        assert bad is None, (f"{what}: the window of input rows {y0} .. {y1 - 1}, columns {x0} .. {x1 - 1} around output ({oy}, {ox}) "
                             f"differs from the oracle, first at (row {yoff + ylo + bad[0]}, x {xoff + xlo + bad[1]}, channel {bad[2]})")


# ---- A: one image just under the limit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lt.SINGLE))
def test_one_image_just_under_2_gib(api, name):
    kinds, w, h, options, kind, family, _, _ = lt.SINGLE[name]
    d = lt.desc(kinds[0], w, h)
    plan = _plan(d, 1, **options)
    assert plan[2:4] == [kind, family], plan
    assert max(lt.tensor_bytes(kinds, w, h)) < lt.L
    wb = lt.chain_weights(kinds, SEED)
    dw, = _device_weights(api, kinds, wb)
    x = _random((1,) + d.in_shape, SEED)
    buf, out = _guarded((1,) + d.out_shape)
    _layer(api, kinds[0], dw, x, w, h, out, options or None)
    torch.cuda.synchronize()
    assert _guards_intact(buf), name
    _windows(kinds, wb, x[0], out[0], w, h, name)
    lt.check_bands(kinds, h, N_BANDS, out[0], lambda a, b: _layer(api, kinds[0], dw, x[:, a:b], w, b - a)[0], name)


def _gdn_objects(api, gdn):
    return None if gdn is None else [None if g is None else api.GDN(*g) for g in gdn]


def _net(api, kinds, w, h, dws, options, gdn=None):
    return api.EightLayersNet(descs=lt.chain_descs(kinds, w, h), shared_weights=dws, options=options, gdn=gdn)


def _chain_case(api, kinds, n, w, h, n_dead, options, columns, halves, groups, what, gdn=None, images=(0,), window_image=0):
    """a chain on n images of w x h as one net call, everything that says what runs asserted first; bands on `images`, windows on one"""
    wb = lt.chain_weights(kinds, SEED, n_dead)
    dws = _device_weights(api, kinds, wb)
    gobj = _gdn_objects(api, gdn)
    net = _net(api, kinds, w, h, dws, options, gobj)
    last = len(kinds) - 1
    c, live = _net_ints("sicn_debug_net_columns", net, n, (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)())
    assert c == [columns] * last + [8] and live[:last] == [128 - n_dead] * last, (c, live)
    hv, = _net_ints("sicn_debug_net_input_halves", net, n, (ctypes.c_int32 * 8)())
    assert hv == [2] * last + [halves], hv
    go, gi = _net_ints("sicn_debug_net_groups", net, n, (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)())
    assert go == [groups] + [4] * last and gi == [4] + [groups] * last, (go, gi)
    x = _random((n,) + net.descs[0].in_shape, SEED + 1)
    buf, out = _guarded((n,) + net.descs[-1].out_shape)
    ws = net.workspace(n)
    ws.fill_(FILL)
    net.run_layers(0, last, x, out=out)
    torch.cuda.synchronize()
    assert _guards_intact(buf), what
    _windows(kinds, wb, x[window_image], out[window_image], w, h, what, gdn, last_rows=True)
    bands = {}

    def run_band(img):
        def run(a, b):
            if b - a not in bands:                      # a net per band height; the library's own choice of kernels (default options)
                bands[b - a] = _net(api, kinds, w, b - a, dws, None, gobj)
            return bands[b - a].run_layers(0, last, x[img:img + 1, a:b])[0][0]
        return run
    for img in images:
        lt.check_bands(kinds, h, N_BANDS, out[img], run_band(img), f"{what}, image {img}")
    return net


@pytest.mark.parametrize("name", list(lt.CHAINS))
def test_internal_layouts_at_the_limit(api, name):
    """conv 3 -> 128 writes GROUP for the wide conv to read at L - 524 288 (three groups where the consumer reads 48 channels); the
    wide deconv stores PHASE at L - 1 048 576 for layer 7, which reads both halves or, behind 3 columns, one"""
    kinds, w, h, n_dead, _ = lt.CHAINS[name]
    assert lt.tensor_bytes(kinds, w, h)[1] in (lt.L - 524288, lt.L - 1048576)
    first_live = kinds[0] != "l0" and n_dead == 80
    assert _plan(lt.desc(kinds[0], w, h), 1)[2:4] == ([3, 0] if kinds[0] == "l0" else [2, 2])
    _chain_case(api, kinds, 1, w, h, n_dead, {}, columns=3 if first_live else 8, halves=1 if first_live else 2,
                groups=3 if kinds[0] == "l0" and n_dead >= 32 else 4, what=name)


def test_l0_writes_three_groups_at_the_limit(api):
    kinds, w, h = ("l0", "conv"), 8192, 8190
    _chain_case(api, kinds, 1, w, h, 80, {}, columns=8, halves=2, groups=3, what="l0 (3 groups) -> conv")


def test_igdn_walks_a_phase_map_at_the_limit(api):
    """the deconv -> layer 7 chain with an IGDN in place of the first layer's ReLU: k_gdn rewrites the PHASE tensor of L - 1 048 576
    bytes in place"""
    kinds, w, h = ("deconv", "rgb"), 2048, 2047
    beta, gamma = lt.gdn_params(128, SEED)
    _chain_case(api, kinds, 1, w, h, 0, {}, columns=8, halves=2, groups=4, what="deconv + IGDN -> layer 7",
                gdn=[(beta, gamma, True, 12), None])


# ---- B: one step over ------------------------------------------------------------------------------------------------------------------
def _raw_call(api, d, dw, x, out, n, options=None):
    L = _lib().lib()
    fn = L.sicn_deconv522_opt if d.transposed else L.sicn_conv2d_opt
    return fn(ctypes.byref(d.to_c()), dw.handle, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), n,
              api._opt_ptr(options), api._stream_ptr(None))


@pytest.mark.parametrize("name", list(lt.SINGLE))
def test_one_row_more_is_refused(api, name):
    """the shapes of A one row higher: exactly L bytes on the side that was L minus one row.  The buffers have their true sizes, so a
    missing check shows as a return code of 0, not as an access outside an allocation."""
    kinds, w, h, options, _, _, _, _ = lt.SINGLE[name]
    d = lt.desc(kinds[0], w, h + 1)
    assert max(lt.tensor_bytes(kinds, w, h + 1)) == lt.L
    dw, = _device_weights(api, kinds, lt.chain_weights(kinds, SEED))
    x = torch.full((1,) + d.in_shape, 0x11, dtype=torch.uint8, device="cuda")
    buf, out = _guarded((1,) + d.out_shape, 0xA5)
    rc = _raw_call(api, d, dw, x, out, 1, options or None)
    torch.cuda.synchronize()
    assert rc == EINVAL, (name, rc)
    assert _all_bytes_are(out, 0xA5) and _guards_intact(buf), name


def test_65536_images_are_refused(api):
    kinds = ("conv",)
    d = lt.desc("conv", 1, 1)
    dw, = _device_weights(api, kinds, lt.chain_weights(kinds, SEED))
    x = torch.full((65536,) + d.in_shape, 0x11, dtype=torch.uint8, device="cuda")
    buf, out = _guarded((65536,) + d.out_shape, 0xA5)
    assert _raw_call(api, d, dw, x, out, 65536) == EINVAL
    torch.cuda.synchronize()
    assert _all_bytes_are(out, 0xA5) and _guards_intact(buf)


def test_rgb_batch_limit(api):
    """87 images of 3840 x 2160 x 3 are 2 164 838 400 bytes: with the 4 bytes a dword load may reach past the end, not below L.  The
    output keeps its true size, 23.1 GB that nothing touches, so that a missing check could not write outside an allocation: the one
    allocation of this file above 8 GiB.  The accepted side, 86 images, would fill 22.8 GB and is left out."""
    n, w, h = 87, 3840, 2160
    assert n * w * h * 3 + 4 >= lt.L > (n - 1) * w * h * 3 + 4
    d = lt.desc("l0", w, h)
    assert _plan(d, n)[2] == 3
    dw, = _device_weights(api, ("l0",), lt.chain_weights(("l0",), SEED))
    x = torch.full((n,) + d.in_shape, 0x11, dtype=torch.uint8, device="cuda")
    out = torch.empty((n,) + d.out_shape, dtype=torch.uint8, device="cuda")
    rc = _raw_call(api, d, dw, x, out, n)
    torch.cuda.synchronize()
    assert rc == EINVAL, rc


def test_a_net_returns_the_refusal_of_its_first_layer_that_refuses(api):
    """deconv 128 -> 128 twice on 1024 x 1024: the first layer's tensors are 128 MiB and 512 MiB, the second one's output is exactly L.
    sicn_net_forward makes no check of its own ahead of the launches: layer 0 is enqueued and runs, layer 1 refuses, the call returns
    its SICN_EINVAL and `out` is untouched."""
    kinds, w, h = ("deconv", "deconv"), 1024, 1024
    assert lt.tensor_bytes(kinds, w, h) == [1 << 27, 1 << 29, lt.L]
    dws = _device_weights(api, kinds, lt.chain_weights(kinds, SEED))
    net = _net(api, kinds, w, h, dws, None)
    x = _random((1,) + net.descs[0].in_shape, SEED)
    buf, out = _guarded((1,) + net.descs[1].out_shape, 0xA5)
    ws = net.workspace(1)
    ws.fill_(FILL)
    rc = _lib().lib().sicn_net_forward(net._h, 0, 1, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), -1, None, 1,
                                       ctypes.c_void_p(ws.data_ptr()), ws.numel(), api._stream_ptr(None))
    torch.cuda.synchronize()
    assert rc == EINVAL, rc
    assert _all_bytes_are(out, 0xA5) and _guards_intact(buf)
    assert not _all_bytes_are(ws, FILL)                 # layer 0 ran into the workspace


# ---- C: image bases on both sides of 2^32 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lt.BATCHES))
def test_image_bases_on_both_sides_of_4_gib(api, name):
    kinds, n, w, h, side = lt.BATCHES[name]
    d = lt.desc(kinds[0], w, h)
    per = lt.tensor_bytes(kinds, w, h)[0 if side == "in" else 1]
    assert (n - 1) * per > lt.G4 and _plan(d, n)[2:4] == list(lt.SINGLE[name][4:6])
    wb = lt.chain_weights(kinds, SEED)
    dw, = _device_weights(api, kinds, wb)
    x = _random((n,) + d.in_shape, SEED + 2)
    assert not torch.equal(x[0], x[n - 1])
    buf, out = _guarded((n,) + d.out_shape)
    _layer(api, kinds[0], dw, x, w, h, out)
    torch.cuda.synchronize()
    assert _guards_intact(buf), name
    straddler = lt.G4 // per
    _windows(kinds, wb, x[straddler], out[straddler], w, h, f"{name}, image {straddler}")
    for img in (0, n - 2, n - 1):
        lt.check_bands(kinds, h, N_BANDS, out[img], lambda a, b: _layer(api, kinds[0], dw, x[img:img + 1, a:b], w, b - a)[0],
                       f"{name}, image {img}")


# ---- D: ragged tensors past 2^32 ------------------------------------------------------------------------------------------------------
# kind, the side whose 128-channel tensor passes 2^32, the kernel, the images (W, H) at the layer's input
RAGGED = {
    "conv": ("conv", "in", "mfma_conv_any", lt.RAGGED_SIZES),
    "deconv": ("deconv", "out", "mfma_deconv_any", lt.RAGGED_HALVES),
    "rgb-conv": ("l0", "out", "mfma_conv_rgb_packed", [(2 * w, 2 * h) for w, h in lt.RAGGED_SIZES]),
    "rgb-deconv": ("rgb", "in", "mfma_deconv_rgb_packed", lt.RAGGED_SIZES),
}


@pytest.mark.parametrize("name", list(RAGGED))
def test_ragged_layer_with_a_tensor_past_4_gib(api, name):
    """one launch over five images; in the 128-channel tensor image 2 begins below 2^32 (at 4 293 918 720; behind the deconv, whose
    images are 4096 x 4094, at 4 292 870 144) and ends past it, images 3 and 4 begin beyond it.  Every image against the per-layer entry point on that image alone (another kernel family): the two big ones
    by bands, the small ones whole, and those against the oracle as well."""
    kind, side, kernel, sizes = RAGGED[name]
    kinds = (kind,)
    wb = lt.chain_weights(kinds, SEED)
    dws = _device_weights(api, kinds, wb)
    net = api.RaggedNet(sizes, descs=lt.chain_descs(kinds, 8, 8), shared_weights=dws)
    assert net.kernel_for(0) == kernel
    big = net._offsets[0 if side == "in" else 1]
    assert big[2] in (4293918720, 4292870144) and big[2] < lt.G4 < big[3] < big[4] < net.nbytes(-1 if side == "in" else 0)
    x = _random((net.nbytes(-1),), SEED + 3)
    buf, out = _guarded((net.nbytes(0),))
    net.run_layers(0, 0, x, out=out)
    torch.cuda.synchronize()
    assert _guards_intact(buf), name
    for i, ((w, h), xi, yi) in enumerate(zip(sizes, net.views(-1, x), net.views(0, out))):
        what = f"{name}, image {i} ({w} x {h})"
        if i < 2:
            lt.check_bands(kinds, h, N_BANDS, yi, lambda a, b: _layer(api, kind, dws[0], xi[None, a:b], w, b - a)[0], what)
        else:
            alone = _layer(api, kind, dws[0], xi[None], w, h)[0]
            assert lt.first_difference(yi, alone) is None, (what, lt.first_difference(yi, alone))
            want = lt.oracle_chain(kinds, wb, xi.cpu().numpy())
            assert lt.first_difference(yi.cpu().numpy(), want) is None, (what, "oracle", lt.first_difference(yi.cpu().numpy(), want))


def test_ragged_crop_and_cut_over_a_tensor_past_4_gib(api):
    """every image of the 4.3 GB tensor cut to its top-left half (RaggedCrop) and to a rectangle at its bottom-right (RaggedCut),
    against torch slicing, exactly and in full"""
    shapes = [(h, w) for w, h in lt.RAGGED_SIZES]
    src_bytes = sum(h * w * 128 for h, w in shapes)
    assert src_bytes > lt.G4
    x = _random((src_bytes,), SEED + 4)
    crop = api.RaggedCrop(shapes, [((h + 1) // 2, (w + 1) // 2) for h, w in shapes], 128)
    rects = [(w - (w + 1) // 2, h - (h + 1) // 2, (w + 1) // 2, (h + 1) // 2) for h, w in shapes]
    cut = api.RaggedCut(shapes, rects, 128)
    assert crop.src_bytes == cut.src_bytes == src_bytes and crop._src_off[2] == 4293918720 and crop._src_off[3] > lt.G4
    src = crop.views(x, "src")
    for op, corners in ((crop, [(0, 0)] * len(shapes)), (cut, [(r[0], r[1]) for r in rects])):
        buf, dst = _guarded((op.dst_bytes,))
        op.run(x, dst)
        torch.cuda.synchronize()
        assert _guards_intact(buf)
        for i, (v, (x0, y0)) in enumerate(zip(op.views(dst), corners)):
            rh, rw, _ = v.shape
            assert torch.equal(v, src[i][y0:y0 + rh, x0:x0 + rw]), (type(op).__name__, i)
        del buf, dst


# ---- E: GDN over lanes ----------------------------------------------------------------------------------------------------------------
PIECE = 1 << 20


@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
@pytest.mark.parametrize("c, chunks, extra", [(128, 1, 300), (128, 2, 1), (192, 1, 300), (192, 2, 1)])
def test_gdn_apply_over_more_than_one_chunk(api, c, chunks, extra, inverse):
    """sicn_gdn_apply cuts its lanes into launches of (2^31 - 4096) / C positions: a second chunk of 300 positions, and a third of 1.
    In full against the same call on pieces of 2^20 positions (one launch each, low offsets); against the oracle on 256 positions at
    the start, at every chunk seam and at the end.  The call works in place, so the input is drawn piece by piece from seeds that
    give every piece again."""
    from oracle import c_oracle
    chunk = lt.gdn_chunk(c)
    n = chunks * chunk + extra
    assert n * c > chunks * (lt.L - 4096) and (chunks < 2 or n * c > lt.G4 - 2 * 4096 - 2 * c)
    beta, gamma = lt.gdn_params(c, SEED)
    g = api.GDN(beta, gamma, inverse, 12)
    buf, lanes = _guarded((n, c))
    starts = list(range(0, n, PIECE))

    def piece(i):
        return _random((min(PIECE, n - starts[i]), c), 1000 * SEED + i)
    for i, s in enumerate(starts):
        lanes[s:s + PIECE] = piece(i)
    spots = sorted({0, n - 256} | {k * chunk - 128 for k in range(1, chunks + 1)})
    before = [lanes[s:s + 256].cpu().numpy() for s in spots]
    g.apply_(lanes)
    torch.cuda.synchronize()
    assert _guards_intact(buf)
    for s, xin in zip(spots, before):
        want = c_oracle.gdn(xin, beta, gamma, inverse, 12)
        assert np.array_equal(lanes[s:s + 256].cpu().numpy(), want), f"positions {s} .. {s + 255} of {n} differ from the oracle"
    for i, s in enumerate(starts):
        want = g.apply_(piece(i))
        if not torch.equal(lanes[s:s + PIECE], want):
            p, ch = (int(v) for v in torch.nonzero(lanes[s:s + PIECE] != want)[0])
            raise AssertionError(f"position {s + p} of {n} (chunk of {chunk}), channel {ch}: got {int(lanes[s + p, ch])} want {int(want[p, ch])}")


# ---- F: NT stores at the smallest size that selects them ----------------------------------------------------------------------
@pytest.mark.parametrize("grid", [0, 16])
@pytest.mark.parametrize("cols", [3, 5, 8])
@pytest.mark.parametrize("name", list(lt.NT_CHAINS))
def test_nt_stores_of_the_wide_and_live_kernels(api, name, cols, grid):
    """the producer of a two-layer chain writes 128 MiB (conv: 2 x 64 MiB, the threshold itself) or more: k_conv_x / k_deconv_x and
    k_conv_live / k_deconv_live<true, 3 | 5> (csrc/k_common.hpp nt_store_wanted), with random weights, so that a channel which lands
    in another column is seen"""
    kinds, n, w, h = lt.NT_CHAINS[name]
    assert n * lt.tensor_bytes(kinds, w, h)[1] >= lt.NT_MIN_BYTES
    options = {"wave_tile": 128, "persistent_grid": grid}
    plan = _plan(lt.desc(kinds[0], w, h), n, **options)
    assert plan[3] == 2 and plan[7] == (grid or _chip()[0]), plan
    _chain_case(api, kinds, n, w, h, lg.N_DEAD[cols], options, columns=cols, halves=1 if kinds[1] == "rgb" and cols == 3 else 2, groups=4,
                what=f"{name}, {cols} columns, grid {grid}", images=range(n), window_image=n - 1)
