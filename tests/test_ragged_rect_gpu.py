"""GPU parity of the rectangle output of a ragged net (include/sicn_ragged_rect.h; run with -m gpu on an MI355X): the deconv N -> 3
whose epilogue stores a rectangle of every reconstruction, interleaved or planar, at origins of the net's own or read from device
memory when the kernel runs, and the ROI decodes made with it (`roi_layout=`, `direct=`).  Everything is byte equality — the path
is integer.  The reference in every case is the interleaved PACKED net on the same weight handles, its full output sliced — and
permuted for planar — on the host; single layers are also held to the C oracle's direct form; an ROI object is held to the same
object made with defaults.  Every forward of this file runs between guard bands of 256 patterned bytes on both sides of `out` and
`tap_out`, over outputs that were filled with random bytes, so that a byte written outside and a byte not written both show."""
import ctypes

import numpy as np
import pytest

from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import CLayerDesc, LayerDesc, eight_layer_descs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = [(1, 1), (16, 16), (17, 33), (35, 35), (100, 36), (131, 70), (33, 1), (2, 67)]      # (width, height), as the planar tests
DECONV_MAPS = [(1, 1), (16, 16), (17, 15), (33, 2), (2, 33), (50, 18)]
GUARD = 256
PATTERN = ((np.arange(GUARD) * 37 + 11) & 255).astype(np.uint8)
EINVAL = -22
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
LAYOUTS = ["interleaved", "planar"]
NAME = {"interleaved": "mfma_deconv_rgb_rect", "planar": "mfma_deconv_rgb_planar_rect"}


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


def _deconv_desc(n, w=16, h=16):
    return LayerDesc.make(n, 3, 8, 3, w, h, 1)


@pytest.fixture(scope="module")
def eight(api):
    rng = np.random.default_rng([411, 128, 192])
    return [_weights_of(api, d, rng)[0] for d in eight_layer_descs(16, 16)]


@pytest.fixture(scope="module")
def param(api):
    return [api.DeviceWeights(d, w, b) for d, (w, b) in zip(eight_layer_descs(16, 16), api.load_param_weights())]


def _guarded(api, net, first, last, xin, tap_layer=-1, origins=None, stream=None):
    """sicn_ragged_net_forward_at into buffers between guard bands, over random bytes; returns (out, tap or None, what `out` held
    before) without the bands."""
    def buf(n):
        t = torch.randint(0, 256, (n + 2 * GUARD,), dtype=torch.uint8, device="cuda")
        t[:GUARD] = torch.from_numpy(PATTERN).cuda()
        t[-GUARD:] = torch.from_numpy(PATTERN).cuda()
        return t
    out = buf(net.nbytes(last))
    before = out[GUARD:-GUARD].clone()
    tap = buf(net.nbytes(tap_layer)) if tap_layer >= 0 else None
    ws = net.workspace()
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = api._lib.lib().sicn_ragged_net_forward_at(
        net._h, first, last, ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr() + GUARD), tap_layer,
        ctypes.c_void_p(tap.data_ptr() + GUARD if tap is not None else 0), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
        ctypes.c_void_p(origins.data_ptr() if origins is not None else 0), ctypes.c_void_p(s.cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    pat = torch.from_numpy(PATTERN).cuda()
    for name, t in (("out", out), ("tap_out", tap)):
        if t is not None:
            assert torch.equal(t[:GUARD], pat), f"bytes in front of {name} were written"
            assert torch.equal(t[-GUARD:], pat), f"bytes behind {name} were written"
    return out[GUARD:-GUARD], (tap[GUARD:-GUARD] if tap is not None else None), before


def _as(layout, x):
    """[h][w][3] -> the layout's array, contiguous (numpy)."""
    return np.ascontiguousarray(x.transpose(2, 0, 1)) if layout == "planar" else np.ascontiguousarray(x)


def _shape(layout, w, h):
    return (3, h, w) if layout == "planar" else (h, w, 3)


def _fit(x0, y0, w, h, W, H):
    """The rectangle moved and shrunk into a W x H reconstruction."""
    x0, y0 = min(x0, W - 1), min(y0, H - 1)
    return (x0, y0, max(1, min(w, W - x0)), max(1, min(h, H - y0)))


# One rectangle per image of kind k, for reconstructions of sizes `rule`: the whole, 1 x 1 at each corner, edges at output columns /
# rows 31 / 32 / 33 (from the corner up to there, and from there to the end), an odd origin with odd sizes, inside one tile.
RECT_KINDS = {
    "whole": lambda W, H: (0, 0, W, H),
    "corner00": lambda W, H: (0, 0, 1, 1),
    "corner10": lambda W, H: (W - 1, 0, 1, 1),
    "corner01": lambda W, H: (0, H - 1, 1, 1),
    "corner11": lambda W, H: (W - 1, H - 1, 1, 1),
    "upto31x32": lambda W, H: _fit(0, 0, 31, 32, W, H),
    "upto32x33": lambda W, H: _fit(0, 0, 32, 33, W, H),
    "upto33x31": lambda W, H: _fit(0, 0, 33, 31, W, H),
    "from31x32": lambda W, H: _fit(31, 32, W, H, W, H),
    "from32x33": lambda W, H: _fit(32, 33, W, H, W, H),
    "from33x31": lambda W, H: _fit(33, 31, W, H, W, H),
    "odd": lambda W, H: _fit(1, 3, (W - 2) | 1, (H - 4) | 1, W, H),
    "odd2": lambda W, H: _fit(3, 1, 5, 3, W, H),
    "in_tile": lambda W, H: _fit(34, 3, 7, 9, W, H),
}


# ---- single-layer deconv, both layouts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 96, 192])
def test_single_deconv_rectangles_both_layouts(api, n):
    """96: a half-empty last K chunk.  The reference runs once; every kind of rectangle then makes a net per layout."""
    rng = np.random.default_rng([421, n])
    dev, words, bias = _weights_of(api, _deconv_desc(n), rng)
    ref = api.RaggedNet(DECONV_MAPS, shared_weights=[dev], descs=[_deconv_desc(n)])
    xs = [rng.integers(0, 256, shp, dtype=np.uint8) for shp in ref.shapes(-1)]
    xin = ref.pack([torch.from_numpy(x) for x in xs])
    want = [v.cpu().numpy() for v in ref.views(0, _guarded(api, ref, 0, 0, xin)[0])]
    for i, x in enumerate(xs):
        o = c_oracle.run_layer(_deconv_desc(n, *DECONV_MAPS[i]), words, bias, x, "direct", threads=16)
        assert np.array_equal(want[i], o), f"image {i}: the reference differs from the oracle"
    assert sum(np.count_nonzero(w) for w in want) > sum(w.size for w in want) // 8
    rule = [(2 * w, 2 * h) for w, h in DECONV_MAPS]
    row_phases = {layout: set() for layout in LAYOUTS}
    plane_phases = set()
    for kind, make in RECT_KINDS.items():
        rects = [make(W, H) for W, H in rule]
        for layout in LAYOUTS:
            net = api.RaggedNet(DECONV_MAPS, shared_weights=[dev], descs=[_deconv_desc(n)], rgb_layout=layout, out_rects=rects)
            assert net.kernel_for(0) == NAME[layout] and net.planar_out == (layout == "planar") and not net.planar_in
            assert net.shapes(0) == [_shape(layout, r[2], r[3]) for r in rects] and net.nbytes(0) == sum(3 * r[2] * r[3] for r in rects)
            got, _, _ = _guarded(api, net, 0, 0, xin)
            for i, ((x0, y0, w, h), v) in enumerate(zip(rects, net.views(0, got))):
                assert v.is_contiguous() and tuple(v.shape) == _shape(layout, w, h)
                assert np.array_equal(v.cpu().numpy(), _as(layout, want[i][y0:y0 + h, x0:x0 + w])), \
                    f"{kind} {layout} image {i}: map {DECONV_MAPS[i]} rectangle {rects[i]}"
            for o, (_, _, w, h) in zip(net._offsets[1], rects):
                if layout == "planar":
                    plane_phases |= {(o + c * w * h) % 4 for c in range(3)}
                    row_phases[layout] |= {(o + (c * h + y) * w) % 4 for c in range(3) for y in range(min(h, 4))}
                else:
                    row_phases[layout] |= {(o + 3 * y * w) % 4 for y in range(min(h, 4))}
    assert plane_phases == {0, 1, 2, 3} and all(p == {0, 1, 2, 3} for p in row_phases.values())


# ---- origins from the device ----------------------------------------------------------------------------------------------------------
def _expected_at(layout, want, before, net, rects, origins):
    """What boundary 0 must hold after a forward at `origins`: the reference's pixel where the rectangle lies inside the
    reconstruction, what the tensor held before everywhere else."""
    exp = before.cpu().numpy().copy()
    for i, ((_, _, w, h), (x0, y0)) in enumerate(zip(rects, origins)):
        H, W, _ = want[i].shape
        o = net._offsets[1][i]
        img = exp[o:o + 3 * w * h].reshape(_shape(layout, w, h))
        ys = [y for y in range(h) if 0 <= y0 + y < H]
        xs = [x for x in range(w) if 0 <= x0 + x < W]
        if not ys or not xs:
            continue
        src = want[i][y0 + ys[0]:y0 + ys[-1] + 1, x0 + xs[0]:x0 + xs[-1] + 1]
        if layout == "planar":
            img[:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = src.transpose(2, 0, 1)
        else:
            img[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = src
    return exp


@pytest.fixture(scope="module")
def moved(api):
    """One deconv 96 -> 3 over DECONV_MAPS, its reference output, and rectangles of fixed sizes per image."""
    rng = np.random.default_rng(431)
    dev, _, _ = _weights_of(api, _deconv_desc(96), rng)
    ref = api.RaggedNet(DECONV_MAPS, shared_weights=[dev], descs=[_deconv_desc(96)])
    xin = ref.pack([torch.from_numpy(rng.integers(0, 256, shp, dtype=np.uint8)) for shp in ref.shapes(-1)])
    out, _ = ref.run_layers(0, 0, xin)
    torch.cuda.synchronize()
    want = [v.cpu().numpy() for v in ref.views(0, out)]
    rule = [(2 * w, 2 * h) for w, h in DECONV_MAPS]
    rects = [(0, 0, 1, 1), (3, 5, 21, 13), (1, 1, 33, 7), (30, 0, 9, 4), (0, 31, 3, 35), (64, 2, 36, 34)]
    return dev, xin, want, rule, rects


def _origin_sets(rule, rects):
    rng = np.random.default_rng(433)
    inside = [(int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))) for (W, H), (_, _, w, h) in zip(rule, rects)]
    return {
        "creation": [(x0, y0) for x0, y0, _, _ in rects],
        "inside": inside,
        "far_corner": [(W - w, H - h) for (W, H), (_, _, w, h) in zip(rule, rects)],
        "partly_left_up": [(-(w // 2) - 1, -(h // 2)) for _, _, w, h in rects],
        "partly_right_down": [(W - w // 2, H - (h + 1) // 2) for (W, H), (_, _, w, h) in zip(rule, rects)],
        "just_outside": [(W, 0) if i % 2 else (-w, 0) for i, ((W, H), (_, _, w, h)) in enumerate(zip(rule, rects))],
        "mixed": [(inside[i] if i % 3 == 0 else (-1, H - 1) if i % 3 == 1 else (W - 1, -1)) for i, (W, H) in enumerate(rule)],
        "int32_min": [(INT32_MIN, INT32_MIN)] * len(rects),
        "int32_max": [(INT32_MAX, INT32_MAX)] * len(rects),
        "int32_both": [(INT32_MIN, INT32_MAX) if i % 2 else (INT32_MAX, 0) for i in range(len(rects))],
    }


@pytest.mark.parametrize("layout", LAYOUTS)
def test_origins_read_from_device_memory(api, moved, layout):
    dev, xin, want, rule, rects = moved
    net = api.RaggedNet(DECONV_MAPS, shared_weights=[dev], descs=[_deconv_desc(96)], rgb_layout=layout, out_rects=rects)
    for name, origins in _origin_sets(rule, rects).items():
        dev_origins = torch.tensor(origins, dtype=torch.int32, device="cuda")
        got, _, before = _guarded(api, net, 0, 0, xin, origins=dev_origins)
        exp = _expected_at(layout, want, before, net, rects, origins)
        assert np.array_equal(got.cpu().numpy(), exp), f"{layout} origins {name}"
        if name.startswith("int32") or name == "just_outside":
            assert torch.equal(got, before), f"{layout} origins {name}: something was written"
        if name == "creation":
            assert torch.equal(net.run_layers(0, 0, xin)[0], net.run_layers(0, 0, xin, origins=dev_origins)[0])
    # tap_out at the last layer is laid out as out is, and moves with it
    origins = _origin_sets(rule, rects)["inside"]
    out, tap, _ = _guarded(api, net, 0, 0, xin, tap_layer=0, origins=torch.tensor(origins, dtype=torch.int32, device="cuda"))
    assert torch.equal(out, tap)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_captured_forward_replays_with_origins_rewritten_on_the_device(api, moved, layout):
    dev, xin, want, rule, rects = moved
    net = api.RaggedNet(DECONV_MAPS, shared_weights=[dev], descs=[_deconv_desc(96)], rgb_layout=layout, out_rects=rects)
    sets = _origin_sets(rule, rects)
    origins = torch.tensor(sets["creation"], dtype=torch.int32, device="cuda")
    out = torch.empty(net.nbytes(0), dtype=torch.uint8, device="cuda")
    net.run_layers(0, 0, xin, out=out, origins=origins)                    # warm-up: module load
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            net.run_layers(0, 0, xin, out=out, origins=origins, stream=side)
    staged = {k: torch.tensor(v, dtype=torch.int32, device="cuda") for k, v in sets.items()}
    for name in ("inside", "partly_left_up", "far_corner", "int32_min", "creation"):
        out.random_(0, 256)
        before = out.clone()
        origins.copy_(staged[name])                                         # device to device: the graph reads what is there now
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), _expected_at(layout, want, before, net, rects, sets[name])), f"{layout} replay at {name}"


# ---- layers 4 .. 7 --------------------------------------------------------------------------------------------------------------------
def _rects_of_sizes(sizes):
    """Per image of SIZES a rectangle of its 16-rounded reconstruction: the image itself (the crop), then interior ones with odd
    corners and sizes."""
    out = []
    for i, (w, h) in enumerate(sizes):
        W, H = 16 * -(-w // 16), 16 * -(-h // 16)
        out.append([(0, 0, w, h), _fit(1, 3, (W // 2) | 1, (H // 2) | 1, W, H), _fit(W // 3, H // 3, 37, 21, W, H)][i % 3])
    return out


def _main_gdn(api):
    from simple_image_compression_network_amd import hyperprior
    gdn = [None if g is None else api.GDN(g[0], g[1], inverse=g[2], shift=g[3]) for g in hyperprior.hyper_parameters(16, 16, 0, True)["gdn_np"]]
    assert gdn[4] is not None and gdn[7] is None
    return gdn


@pytest.mark.parametrize("weights,with_gdn", [("random", False), ("param", False), ("param", True), ("random", True)])
def test_layers_four_to_seven_from_the_references_latent(api, eight, param, weights, with_gdn):
    dev = eight if weights == "random" else param
    gdn = _main_gdn(api) if with_gdn else None
    ref = api.RaggedNet(SIZES, shared_weights=dev, gdn=gdn)
    images = [np.random.default_rng([437, i]).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (w, h) in enumerate(SIZES)]
    xin = ref.pack([torch.from_numpy(x) for x in images])
    w_out, lat = ref.forward(xin)
    torch.cuda.synchronize()
    want = [v.cpu().numpy() for v in ref.views(7, w_out)]
    assert np.count_nonzero(lat.cpu().numpy()) > 0
    rects = _rects_of_sizes(SIZES)
    for layout in LAYOUTS:
        net = api.RaggedNet(SIZES, shared_weights=dev, gdn=gdn, out_rects=rects, out_layout=layout)
        assert net.kernel_for(7) == NAME[layout] and net.kernel_for(0) == "mfma_conv_rgb_packed" and not net.planar_in
        got, _, _ = _guarded(api, net, 4, 7, lat)
        for i, ((x0, y0, w, h), v) in enumerate(zip(rects, net.views(7, got))):
            assert np.array_equal(v.cpu().numpy(), _as(layout, want[i][y0:y0 + h, x0:x0 + w])), f"{layout} image {i} {SIZES[i]} {rects[i]}"
        # all eight layers with the latent tapped: the same bytes
        out8, tap, _ = _guarded(api, net, 0, 7, xin, tap_layer=3)
        assert torch.equal(out8, got) and torch.equal(tap, lat)
        assert net.live_tiles == [(-(-(x0 + w) // 32) - x0 // 32) * (-(-(y0 + h) // 32) - y0 // 32) for x0, y0, w, h in rects]
    # rgb_layout="planar" makes both ends planar, the output at the rectangles
    both = api.RaggedNet(SIZES, shared_weights=dev, gdn=gdn, out_rects=rects, rgb_layout="planar")
    assert both.planar_in and both.planar_out and both.kernel_for(7) == NAME["planar"]
    got, _, _ = _guarded(api, both, 4, 7, lat)
    for i, ((x0, y0, w, h), v) in enumerate(zip(rects, both.views(7, got))):
        assert np.array_equal(v.cpu().numpy(), _as("planar", want[i][y0:y0 + h, x0:x0 + w]))


# ---- the ROI objects ------------------------------------------------------------------------------------------------------------------
ROI_SIZES = [(100, 36), (131, 70), (48, 48), (35, 35)]
ROI_RECTS = [(17, 3, 64, 30), None, (1, 1, 33, 15), (34, 34, 1, 1)]
MOVE_SLOTS = [(0, 33, 15), (1, 20, 31), (1, 64, 40), (2, 16, 16), (3, 1, 1), (0, 100, 36)]
MOVES = [[(0, 0)] * 6, [(5, 7), (100, 30), (60, 29), (31, 32), (34, 34), (0, 0)], [(67, 21), (111, 39), (67, 30), (32, 31), (0, 34), (0, 0)],
         [(-5, 3), (3, -7), (500, 500), (INT32_MIN, INT32_MAX), (INT32_MAX, INT32_MIN), (-1, -1)],                     # clamped
         [(66, 20), (1, 1), (0, 0), (15, 16), (17, 17), (1, 0)], [(67, 22), (112, 40), (68, 31), (33, 33), (35, 35), (0, 1)],   # clamped by one
         [(16, 16), (32, 32), (33, 15), (1, 31), (16, 0), (0, 0)], [(31, 1), (47, 15), (48, 16), (0, 17), (33, 1), (0, 0)],
         [(32, 0), (63, 0), (15, 15), (16, 16), (3, 30), (0, 0)], [(1, 20), (110, 1), (2, 3), (30, 30), (20, 20), (0, 0)],
         [(48, 5), (64, 7), (31, 9), (7, 7), (34, 0), (0, 0)], [(50, 21), (96, 38), (66, 29), (8, 24), (0, 0), (0, 0)]]


def _same_pixels(obj, got, ref_obj, want, layout):
    """`got` of `obj` (direct, in `layout`) against `want` of `ref_obj` (defaults), view by view."""
    a, b = obj.views(got), ref_obj.views(want)
    assert len(a) == len(b)
    for k, (v, r) in enumerate(zip(a, b)):
        assert v.is_contiguous() and tuple(v.shape) == _shape(layout, r.shape[1], r.shape[0])
        assert np.array_equal(v.cpu().numpy(), _as(layout, r.cpu().numpy())), f"view {k}"


@pytest.fixture(scope="module")
def roi_world(api, param):
    """ROI_SIZES on the PARAM weights, with and without the main net's GDN list: the nets, coders with the containers, the archive."""
    made = {}

    def get(with_gdn):
        if with_gdn not in made:
            net = api.RaggedNet(ROI_SIZES, shared_weights=param, gdn=_main_gdn(api) if with_gdn else None)
            xin = net.pack([torch.from_numpy(np.random.default_rng([439, i]).integers(0, 256, (h, w, 3), dtype=np.uint8))
                            for i, (w, h) in enumerate(ROI_SIZES)])
            coder = net.latent_coder(1024)
            coder.encode(net.run_layers(0, 3, xin)[0])
            blob = net.compress_archive(xin, stream_symbols=1024)
            torch.cuda.synchronize()
            made[with_gdn] = (net, coder, blob)
        return made[with_gdn]
    return get


@pytest.mark.parametrize("with_gdn", [False, True])
def test_ragged_roi_and_the_archive_path(api, roi_world, with_gdn):
    net, coder, blob = roi_world(with_gdn)
    base = api.RaggedRoi(net, ROI_RECTS, coder=coder)
    want = base.decode()
    assert base.pixel_cut is not None and not base.direct and base.roi_layout == "interleaved"
    for layout, direct in (("planar", True), ("planar", None), ("interleaved", True)):
        roi = api.RaggedRoi(net, ROI_RECTS, coder=coder, roi_layout=layout, direct=direct)
        assert roi.direct and roi.pixel_cut is None and roi.window_net.kernel_for(7) == NAME[layout]
        out = torch.randint(0, 256, (want.numel(),), dtype=torch.uint8, device="cuda")
        got = roi.decode(out=out)
        assert got.data_ptr() == out.data_ptr()
        _same_pixels(roi, got, base, want, layout)
        assert not roi.status[:, 0].any()
    # interleaved without direct, named: today's chain
    named = api.RaggedRoi(net, ROI_RECTS, coder=coder, roi_layout="interleaved")
    assert not named.direct and torch.equal(named.decode(), want)
    with pytest.raises(ValueError, match="direct"):
        api.RaggedRoi(net, ROI_RECTS, coder=coder, roi_layout="planar", direct=False)
    with pytest.raises(ValueError, match="roi_layout"):
        api.RaggedRoi(net, ROI_RECTS, coder=coder, roi_layout="chw")
    # decompress_archive(rois=)
    want = net.decompress_archive(blob, rois=ROI_RECTS)
    base = net._last_roi
    for layout, direct in (("planar", None), ("interleaved", True)):
        got = net.decompress_archive(blob, rois=ROI_RECTS, roi_layout=layout, direct=direct)
        assert net._last_roi is not base and net._last_roi.direct
        _same_pixels(net._last_roi, got, base, want, layout)
        assert [tuple(v.shape) for v in net.roi_views(got)] == [_shape(layout, *((r[2], r[3]) if r else s)) for r, s in zip(ROI_RECTS, ROI_SIZES)]


def test_a_planar_net_decodes_rois_once_the_layout_is_named(api, param, roi_world):
    net, coder, blob = roi_world(False)
    planar = api.RaggedNet(ROI_SIZES, shared_weights=param, rgb_layout="planar")
    with pytest.raises(ValueError, match="planar"):
        api.RaggedRoi(planar, ROI_RECTS)
    with pytest.raises(ValueError, match="planar"):
        planar.moving_roi([(0, 8, 8)])
    want = net.decompress_archive(blob, rois=ROI_RECTS)
    base = net._last_roi
    for layout in LAYOUTS:
        got = planar.decompress_archive(blob, rois=ROI_RECTS, roi_layout=layout, direct=True)
        _same_pixels(planar._last_roi, got, base, want, layout)


@pytest.mark.parametrize("with_gdn", [False, True])
def test_moving_roi_twelve_moves_graph_and_memory(api, roi_world, with_gdn):
    net, coder, _ = roi_world(with_gdn)
    base = net.moving_roi(MOVE_SLOTS, coder=coder)
    assert base.recon is not None and not base.direct
    wants = []
    for xy in MOVES:
        wants.append(base.decode(xy).clone())
    for layout, direct in (("planar", None), ("interleaved", True)):
        mv = net.moving_roi(MOVE_SLOTS, coder=coder, roi_layout=layout, direct=direct)
        assert mv.direct and mv.recon is None and mv.window_net.kernel_for(7) == NAME[layout]
        mv.decode(MOVES[0])
        got = None                        # the last view of the previous object's pixels is dropped here, not while a decode is watched
        for xy, want in zip(MOVES, wants):
            xy_dev = torch.tensor(xy, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            mv.roi.random_(0, 256)
            before = torch.cuda.memory_allocated()
            got = mv.decode(xy_dev)
            assert torch.cuda.memory_allocated() == before
            _same_pixels(mv, got, base, want, layout)
            assert not mv.status[:, 0].any()
        assert mv.flags.cpu().tolist() == [0] * 6                                   # the last move is inside
        mv.decode(MOVES[3])
        assert mv.flags.cpu().tolist() == [1, 1, 1, 1, 1, 1]
        # positions drawn on the device inside a captured graph
        xy_dev = torch.zeros((6, 2), dtype=torch.int32, device="cuda")
        pool = torch.tensor(MOVES, dtype=torch.int32, device="cuda")
        pick = torch.zeros((), dtype=torch.int64, device="cuda")
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                xy_dev.copy_(pool.index_select(0, pick.reshape(1))[0])
                got = mv.decode(xy_dev, stream=side)
        for k in (7, 3, 11):
            pick.fill_(k)
            mv.roi.random_(0, 256)
            graph.replay()
            torch.cuda.synchronize()
            _same_pixels(mv, got, base, wants[k], layout)
    # uniform slots come back as one array, planes first for planar
    uni = net.moving_roi([(0, 33, 15), (1, 33, 15)], coder=coder, roi_layout="planar")
    ref = net.moving_roi([(0, 33, 15), (1, 33, 15)], coder=coder)
    got, want = uni.decode([(3, 4), (50, 50)]), ref.decode([(3, 4), (50, 50)])
    assert tuple(got.shape) == (2, 3, 15, 33) and torch.equal(got, want.permute(0, 3, 1, 2))


@pytest.mark.parametrize("use_gdn", [False, True])
def test_hyperprior_roi_objects(api, use_gdn):
    from simple_image_compression_network_amd import hyperprior
    rc = hyperprior.RaggedHyperpriorCodec(ROI_SIZES, seed=7, use_gdn=use_gdn, y_stream_symbols=1024)
    rc.encode(rc.main.pack([torch.from_numpy(np.random.default_rng([443, i]).integers(0, 256, (h, w, 3), dtype=np.uint8))
                            for i, (w, h) in enumerate(ROI_SIZES)]))
    rc.check()
    base = rc.roi(ROI_RECTS)
    want = base.decode().clone()
    assert base.pixel_cut is not None
    for layout, direct in (("planar", None), ("interleaved", True)):
        roi = rc.roi(ROI_RECTS, roi_layout=layout, direct=direct)
        assert roi.direct and roi.pixel_cut is None and roi.window_net.kernel_for(7) == NAME[layout]
        got = roi.decode()
        roi.check()
        _same_pixels(roi, got, base, want, layout)
        # decode(rois=)
        got = rc.decode(rois=ROI_RECTS, roi_layout=layout, direct=direct)
        rc.check()
        assert rc._last_roi.direct
        _same_pixels(rc._last_roi, got, base, want, layout)
        assert [tuple(v.shape) for v in rc.roi_views(got)] == [tuple(v.shape) for v in roi.views(got)]
    assert torch.equal(rc.decode(rois=ROI_RECTS), want) and not rc._last_roi.direct
    # MovingHyperpriorRoi
    mbase = rc.moving_roi(MOVE_SLOTS)
    mbase.prepare()
    wants = [mbase.decode(xy).clone() for xy in MOVES]
    for layout, direct in (("planar", None), ("interleaved", True)):
        mv = rc.moving_roi(MOVE_SLOTS, roi_layout=layout, direct=direct)
        assert mv.direct and mv.recon is None
        mv.prepare()
        mv.decode(MOVES[0])
        got = None                        # the last view of the previous object's pixels is dropped here, not while a decode is watched
        for xy, w in zip(MOVES, wants):
            xy_dev = torch.tensor(xy, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            mv.roi.random_(0, 256)
            before = torch.cuda.memory_allocated()
            got = mv.decode(xy_dev)
            assert torch.cuda.memory_allocated() == before
            _same_pixels(mv, got, mbase, w, layout)
        xy_dev = torch.zeros((6, 2), dtype=torch.int32, device="cuda")
        pool = torch.tensor(MOVES, dtype=torch.int32, device="cuda")
        pick = torch.zeros((), dtype=torch.int64, device="cuda")
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                xy_dev.copy_(pool.index_select(0, pick.reshape(1))[0])
                got = mv.decode(xy_dev, stream=side)
        for k in (5, 3, 10):
            pick.fill_(k)
            mv.roi.random_(0, 256)
            graph.replay()
            torch.cuda.synchronize()
            _same_pixels(mv, got, mbase, wants[k], layout)


def test_the_origins_table_of_a_moving_object_is_the_host_placement(api, roi_world):
    net, coder, _ = roi_world(False)
    mv = net.moving_roi(MOVE_SLOTS, coder=coder, roi_layout="planar")
    """Seen through the kernel that reads it: layer 7 of the window net over one random input, at the object's own table and at the
    host placement's corners uploaded as a tensor, gives the same bytes — before the first decode (the placement of (0, 0)) and
    after moves, a clamped one included."""
    L = api._lib.lib()
    ptr = L.sicn_ragged_roi_move_origins(mv._h)
    assert ptr and ptr % 8 == 0 and mv._origins.value == ptr
    wn = mv.window_net
    x6 = torch.randint(0, 256, (wn.nbytes(6),), dtype=torch.uint8, device="cuda")

    def through_the_table(xy):
        want = torch.tensor([(p["x"], p["y"]) for p in mv.place(xy)], dtype=torch.int32, device="cuda")
        a = wn.run_layers(7, 7, x6, origins=mv._origins)[0]
        b = wn.run_layers(7, 7, x6, origins=want)[0]
        torch.cuda.synchronize()
        assert torch.equal(a, b) and a.any()
        return want.cpu().tolist()
    seen = [through_the_table([(0, 0)] * 6)]                                         # before the first decode
    for xy in (MOVES[1], MOVES[3], MOVES[2]):
        mv.decode(xy)
        seen.append(through_the_table(xy))
    assert len({str(s) for s in seen}) > 2                                           # the corners did move


# ---- names and refusals ---------------------------------------------------------------------------------------------------------------
def test_kernel_for_and_every_refusal(api, eight):
    L = api._lib.lib()
    d8 = eight_layer_descs(16, 16)
    n_img = 2
    ws, hs = (ctypes.c_int32 * n_img)(35, 100), (ctypes.c_int32 * n_img)(35, 36)            # reconstructions 48 x 48 and 112 x 48
    good = [(1, 2, 35, 35), (12, 12, 100, 36)]

    def rects_of(r):
        return None if r is None else (api._lib.RaggedRect * n_img)(*[api._lib.RaggedRect(*v) for v in r])

    def create(descs, weights, rects, gdn=None, rgb_ends=1, pin=0, pout=0, keep=False):
        n = len(descs)
        cd = (CLayerDesc * n)(*[d.to_c() for d in descs])
        handles = (ctypes.c_void_p * n)(*[w.handle for w in weights])
        gh = None if gdn is None else (ctypes.c_void_p * n)(*[(g.handle if g is not None else None) for g in gdn])
        h = ctypes.c_void_p(0)
        rc = L.sicn_ragged_net_create_rect(cd, handles, gh, n, ws, hs, n_img, rgb_ends, pin, pout, rects_of(rects), ctypes.byref(h))
        if rc == 0:
            assert h.value
            if keep:
                return h
            L.sicn_ragged_net_free(h)
        else:
            assert not h.value
        return rc
    from simple_image_compression_network_amd import hyperprior
    p3 = hyperprior.random_gdn_params(np.random.default_rng(449), 3)
    igdn = api.GDN(p3[0], p3[1], inverse=True, shift=12)
    for pout in (0, 1):
        assert create(d8, eight, good, pout=pout) == 0 and create(d8, eight, good, pin=1, pout=pout) == 0
        assert create(d8[4:], eight[4:], good, pout=pout) == 0 and create(d8[7:], eight[7:], good, pout=pout) == 0
        assert create(d8, eight, None, pout=pout) == 0                                      # sicn_ragged_net_create_planar without sizes
        assert create(d8[:7], eight[:7], good, pout=pout) == EINVAL                         # the last layer is a deconv 128 -> 128
        assert create(d8[:4], eight[:4], good, pout=pout) == EINVAL                         # ... a conv
        assert create(d8, eight, good, rgb_ends=0, pout=pout) == EINVAL                     # rgb_ends != PACKED
        assert create(d8, eight, good, gdn=[None] * 7 + [igdn], pout=pout) == EINVAL        # an IGDN on the last layer
        for bad in ((0, 0, 0, 1), (0, 0, 1, 0), (0, 0, -3, 1), (-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, 49, 48), (0, 0, 48, 49), (48, 0, 1, 1),
                    (0, 48, 1, 1), (14, 0, 35, 35), (0, 14, 35, 35), (INT32_MAX, 0, 1, 1), (1, 0, INT32_MAX, 1)):
            assert create(d8, eight, [bad, good[1]], pout=pout) == EINVAL, bad
        assert create(d8, eight, good, pout=2) == EINVAL and create(d8, eight, good, pin=2) == EINVAL
        assert create(d8[1:], eight[1:], good, pin=1, pout=pout) == EINVAL                  # what create_planar refuses
    assert create(d8, eight, None, gdn=[None] * 7 + [igdn]) == 0                            # without rectangles an IGDN there is fine
    # names
    for pout, name in ((0, "mfma_deconv_rgb_rect"), (1, "mfma_deconv_rgb_planar_rect")):
        h = create(d8, eight, good, pout=pout, keep=True)
        assert L.sicn_ragged_net_kernel_for(h, 7) == name.encode() and L.sicn_ragged_net_kernel_for(h, 6) == b"mfma_deconv_any"
        assert L.sicn_ragged_net_kernel_for(h, 0) == b"mfma_conv_rgb_packed" and L.sicn_ragged_net_kernel_for(h, 8) is None
        L.sicn_ragged_net_free(h)
    # forward_at
    rect_net = api.RaggedNet([(35, 35), (100, 36)], shared_weights=eight, out_rects=good)
    plain = api.RaggedNet([(35, 35), (100, 36)], shared_weights=eight)
    planar = api.RaggedNet([(35, 35), (100, 36)], shared_weights=eight, rgb_layout="planar")
    origins = torch.zeros(5, dtype=torch.int32, device="cuda")
    vp = ctypes.c_void_p

    def at(net, first, last, optr):
        xin = torch.zeros(net.nbytes(first - 1), dtype=torch.uint8, device="cuda")
        out = torch.zeros(net.nbytes(last), dtype=torch.uint8, device="cuda")
        ws_ = net.workspace()
        rc = L.sicn_ragged_net_forward_at(net._h, first, last, vp(xin.data_ptr()), vp(out.data_ptr()), -1, None, vp(ws_.data_ptr()),
                                          ws_.numel(), vp(optr), None)
        torch.cuda.synchronize()
        return rc, out
    assert at(rect_net, 4, 7, origins.data_ptr())[0] == 0 and at(rect_net, 4, 7, 0)[0] == 0 and at(rect_net, 4, 6, 0)[0] == 0
    assert at(plain, 4, 7, 0)[0] == 0 and at(planar, 4, 7, 0)[0] == 0
    for net in (plain, planar):
        assert at(net, 4, 7, origins.data_ptr())[0] == EINVAL                               # not made with rectangles
    assert at(rect_net, 4, 6, origins.data_ptr())[0] == EINVAL                              # last != n_layers - 1
    for off in (1, 2, 3):
        assert at(rect_net, 4, 7, origins.data_ptr() + off)[0] == EINVAL                    # a misaligned pointer
    assert at(rect_net, 4, 7, origins.data_ptr() + 4)[0] == 0
    with pytest.raises(ValueError, match="origins"):
        plain.run_layers(4, 7, torch.zeros(plain.nbytes(3), dtype=torch.uint8, device="cuda"), origins=origins[:4].view(2, 2))
    with pytest.raises(ValueError, match="origins"):
        rect_net.run_layers(4, 6, torch.zeros(rect_net.nbytes(3), dtype=torch.uint8, device="cuda"), origins=origins[:4].view(2, 2))
    with pytest.raises(TypeError, match="origins"):
        rect_net.run_layers(4, 7, torch.zeros(rect_net.nbytes(3), dtype=torch.uint8, device="cuda"), origins=origins[:4])
