"""GPU checks of the ROI decode (include/sicn_ragged_window.h, csrc/k_ragged_window.hip; run with -m gpu on an MI355X): a pixel
rectangle of each image of a ragged batch decoded from its streams without the rest of the image.  Byte equality throughout; the
reference is the full path of the same containers — RaggedLatentCoder.decode, RaggedNet.decompress / decompress_archive(images=) —
sliced in numpy."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ENOSPC = -28
GUARD = 4096
PATTERN = 0xA5
LAT_C = 192
SIZES_A = [(112, 144), (100, 131), (16, 16), (256, 48)]            # (width, height): latents 7 x 9, 7 x 9, 1 x 1, 16 x 3
# one rectangle per image of batch A and scenario; None = the image whole
SCENARIOS = {
    "interior": [(40, 50, 30, 20), (33, 41, 20, 30), (5, 5, 4, 4), (100, 10, 50, 20)],
    "one-pixel": [(57, 99, 1, 1), (16, 31, 1, 1), (0, 0, 1, 1), (255, 47, 1, 1)],
    "top-left": [(0, 0, 10, 10), (0, 0, 17, 3), (0, 0, 16, 16), (0, 0, 33, 15)],
    "top-right": [(100, 0, 12, 10), (83, 0, 17, 3), (15, 0, 1, 1), (223, 0, 33, 15)],
    "bottom-left": [(0, 134, 10, 10), (0, 128, 17, 3), (0, 15, 1, 1), (0, 33, 33, 15)],
    "bottom-right": [(102, 134, 10, 10), (83, 128, 17, 3), (15, 15, 1, 1), (223, 33, 33, 15)],
    "full-width": [(0, 60, 112, 7), (0, 100, 100, 5), (0, 3, 16, 2), (0, 20, 256, 9)],
    "full-height": [(50, 0, 9, 144), (90, 0, 10, 131), (7, 0, 3, 16), (130, 0, 5, 48)],
    "whole": [None, None, None, None],
    "cropped-edge": [(70, 100, 42, 44), (60, 100, 40, 31), None, (200, 40, 56, 8)],   # image 1: right and bottom edge of 100 x 131 in 112 x 144
}


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import _lib, api, codec
    return _lib, api, codec


@pytest.fixture(scope="module")
def weights(mods):
    _, api, _ = mods
    from simple_image_compression_network_amd.config import eight_layer_descs
    return [api.DeviceWeights(d, w, b) for d, (w, b) in zip(eight_layer_descs(16, 16), api.load_param_weights())]


class Batch:
    """A ragged batch, its containers in a coder's slots, and the full path's results on the host — computed once, never changed."""

    def __init__(self, mods, weights, sizes, wss, seed):
        _, api, _ = mods
        self.sizes, self.wss = sizes, wss
        self.net = api.RaggedNet(sizes, shared_weights=weights)
        rng = np.random.default_rng(seed)
        xin = self.net.pack([torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in sizes])
        self.coder = self.net.latent_coder(wss)
        latent, _ = self.net.run_layers(0, 3, xin)
        self.coder.encode(latent)
        full = torch.empty_like(latent)
        self.coder.decode(full)                                      # the full decoder of the same containers
        recon, _ = self.net.run_layers(4, 7, full)
        torch.cuda.synchronize()
        assert not self.coder.enc_status[:, 0].any() and not self.coder.dec_status[:, 0].any()
        self.latents = [v.cpu().numpy() for v in self.coder.views(full)]
        self.recons = [v.cpu().numpy()[:h, :w] for v, (w, h) in zip(self.net.views(7, recon), sizes)]
        self.enc = self.coder.enc_status.clone()
        self.slots = self.coder.slot_buffer.clone()                  # pristine copies for the tests that damage a container


@pytest.fixture(scope="module")
def batch_a(mods, weights):
    return {wss: Batch(mods, weights, SIZES_A, wss, seed=31) for wss in (1024, 16384)}


def _rect(r, size):
    return (0, 0) + tuple(size) if r is None else r


def _check_band(window, band_host, batch):
    at = 0
    for i, (im, lat) in enumerate(zip(window.images, batch.latents)):
        a, nb, first = int(im.band_offset), int(im.band_bytes), int(im.first_stream)
        flat = lat.reshape(-1)
        assert np.array_equal(band_host[a:a + nb], flat[first * batch.wss:first * batch.wss + nb]), f"image {i}: band differs"
        assert (band_host[at:a] == PATTERN).all(), f"bytes in front of band {i} were written"
        at = a + nb
    assert (band_host[at:] == PATTERN).all()


def test_streams_of_batch_a_are_what_the_issue_counts(mods, batch_a):
    assert [int(im.n_streams) for im in batch_a[1024].coder.images[:4]] == [12, 12, 1, 9]
    assert [int(im.n_streams) for im in batch_a[16384].coder.images[:4]] == [1, 1, 1, 1]
    assert [(h, w) for h, w, _ in batch_a[1024].net.shapes(3)] == [(9, 7), (9, 7), (1, 1), (3, 16)]


@pytest.mark.parametrize("wss", [1024, 16384])
@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_batch_a_stage_by_stage(mods, batch_a, scenario, wss):
    _, api, _ = mods
    b = batch_a[wss]
    rects = SCENARIOS[scenario]
    roi = api.RaggedRoi(b.net, rects, coder=b.coder)
    # 1: the band against the full latent's bytes
    band = torch.full((roi.window.band_bytes,), PATTERN, dtype=torch.uint8, device="cuda")
    roi.window.decode(band)
    torch.cuda.synchronize()
    st = roi.status.cpu().numpy().astype(np.int64)
    assert not st[:, 0].any(), st
    assert st[:, 1].tolist() == [int(im.band_bytes) for im in roi.window.images[:4]]
    _check_band(roi.window, band.cpu().numpy(), b)
    for v, lat, p in zip(roi.window.views(band), b.latents, roi.plans):
        assert np.array_equal(v.cpu().numpy(), lat[p["r0"]:p["r0"] + p["rh"]])
    # 2: the cut latent against numpy slicing
    wlat = roi.latent_cut.run(band)
    torch.cuda.synchronize()
    for i, (v, lat, p) in enumerate(zip(roi.latent_cut.views(wlat), b.latents, roi.plans)):
        assert np.array_equal(v.cpu().numpy(), lat[p["r0"]:p["r0"] + p["rh"], p["c0"]:p["c0"] + p["cw"]]), f"image {i}: window latent differs"
    # 3: the ROI pixels against the sliced full reconstruction, by hand and through decode()
    recon, _ = roi.window_net.run_layers(4, 7, wlat)
    pixels = roi.pixel_cut.run(recon)
    again = roi.decode()
    torch.cuda.synchronize()
    assert torch.equal(pixels, again)
    for i, (v, full, r, size) in enumerate(zip(roi.views(pixels), b.recons, rects, b.sizes)):
        x0, y0, w, h = _rect(r, size)
        assert tuple(v.shape) == (h, w, 3)
        assert np.array_equal(v.cpu().numpy(), full[y0:y0 + h, x0:x0 + w]), f"image {i}: ROI pixels differ from the full decode"
    assert not roi.status[:, 0].any()


def test_window_selects_fewer_streams_than_the_image_has(mods, batch_a):
    """Rows straddle streams in images 0 and 1 (1344 symbols per row, 1024 per stream); in image 3 every second row boundary is a
    stream boundary (3072 symbols per row)."""
    b = batch_a[1024]
    w = b.coder.window([(4, 1), (8, 1), (0, 1), (2, 1)])
    got = [(int(im.first_stream), int(im.end_stream), int(im.lead)) for im in w.images[:4]]
    assert got == [(5, 7, 4 * 1344 - 5 * 1024), (10, 12, 8 * 1344 - 10 * 1024), (0, 1, 0), (6, 9, 0)]
    band = torch.full((w.band_bytes,), PATTERN, dtype=torch.uint8, device="cuda")
    w.decode(band)
    w.check()
    _check_band(w, band.cpu().numpy(), b)
    with pytest.raises(ValueError):
        b.coder.window([(4, 1), (8, 2), (0, 1), (2, 1)])
    with pytest.raises(ValueError):
        b.coder.window([(4, 1)])


# ---- the cut alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [3, 16, 192, 193])
def test_cut_alone_against_numpy_and_crop(mods, channels):
    _, api, _ = mods
    rng = np.random.default_rng(40 + channels)
    shapes = [(9, 7), (21, 16), (1, 1), (8, 40), (17, 3)]            # (h, w): more than one work item of 8 rows, and less
    rects = [(2, 3, 4, 5), (0, 4, 16, 17), (0, 0, 1, 1), (16, 0, 16, 8), (1, 16, 2, 1)]
    src = [rng.integers(0, 256, (h, w, channels), dtype=np.uint8) for h, w in shapes]
    flat = np.concatenate([s.reshape(-1) for s in src])

    def want(rr):
        return np.concatenate([s[y0:y0 + h, x0:x0 + w].reshape(-1) for s, (x0, y0, w, h) in zip(src, rr)])

    cut = api.RaggedCut(shapes, rects, channels)
    assert cut.src_bytes == flat.size
    # aligned and odd base pointers, source and destination independently
    for so, do in ((0, 0), (1, 0), (0, 1), (3, 5)):
        s = torch.full((flat.size + 16,), PATTERN, dtype=torch.uint8, device="cuda")
        s[so:so + flat.size] = torch.from_numpy(flat).cuda()
        d = torch.full((GUARD + cut.dst_bytes + 16 + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        a = GUARD + do
        cut.run(s[so:so + flat.size], d[a:a + cut.dst_bytes])
        torch.cuda.synchronize()
        h = d.cpu().numpy()
        assert np.array_equal(h[a:a + cut.dst_bytes], want(rects)), (so, do)
        assert (h[:a] == PATTERN).all() and (h[a + cut.dst_bytes:] == PATTERN).all(), (so, do)
    for v, s, (x0, y0, w, h) in zip(cut.views(cut.run(torch.from_numpy(flat).cuda())), src, rects):
        assert np.array_equal(v.cpu().numpy(), s[y0:y0 + h, x0:x0 + w])
    # the corner rectangles are the crop
    corner = [(0, 0, max(w - 1, 1), max(h // 2, 1)) for h, w in shapes]
    got = api.RaggedCut(shapes, corner, channels).run(torch.from_numpy(flat).cuda())
    crop = api.RaggedCrop(shapes, [(h, w) for _, _, w, h in corner], channels).run(torch.from_numpy(flat).cuda())
    torch.cuda.synchronize()
    assert torch.equal(got, crop) and np.array_equal(got.cpu().numpy(), want(corner))
    # explicit source offsets: any order, gaps, 16-aligned or not
    align = 16 if channels % 16 == 0 else 1
    offs, at = [0] * len(src), 0
    for i in (3, 0, 4, 2, 1):
        at += 5 * align
        offs[i] = at
        at += src[i].size
    spread = np.full(at + 7, PATTERN, np.uint8)
    for o, s in zip(offs, src):
        spread[o:o + s.size] = s.reshape(-1)
    cut = api.RaggedCut(shapes, rects, channels, src_offsets=offs)
    assert cut.src_bytes == max(o + s.size for o, s in zip(offs, src))
    got = cut.run(torch.from_numpy(spread).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want(rects))
    for bad in ([(2, 3, 6, 5)] + rects[1:], [(2, 3, 0, 5)] + rects[1:], rects[:-1]):
        with pytest.raises(ValueError):
            api.RaggedCut(shapes, bad, channels)


# ---- both forms of the window decode kernel ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch_big(mods, weights):
    return Batch(mods, weights, [(640, 400)] * 8, 1024, seed=32)


def test_full_height_windows_run_the_two_table_form(mods, batch_big):
    _, api, _ = mods
    b = batch_big
    rects = [(300 + 7 * i, 0, 20 + i, 400) for i in range(8)]
    roi = api.RaggedRoi(b.net, rects, coder=b.coder)
    assert roi.window.selected_streams == 8 * 188 == 1504 > 5 * 256           # above 5 x n_cu on a whole chip: k_ragged_decode_window<false>
    pixels = roi.decode()
    torch.cuda.synchronize()
    assert not roi.status[:, 0].any()
    _check_band_plain(roi.window, roi.band.cpu().numpy(), b)
    for i, (v, full, (x0, y0, w, h)) in enumerate(zip(roi.views(pixels), b.recons, rects)):
        assert np.array_equal(v.cpu().numpy(), full[y0:y0 + h, x0:x0 + w]), f"image {i}"


def test_two_row_windows_run_the_one_table_form(mods, batch_big):
    b = batch_big
    w = b.coder.window([(3 * i, 2) for i in range(8)])
    assert w.selected_streams <= 8 * 16 < 5 * 256                             # k_ragged_decode_window<true>
    band = torch.full((w.band_bytes,), PATTERN, dtype=torch.uint8, device="cuda")
    w.decode(band)
    w.check()
    _check_band(w, band.cpu().numpy(), b)
    for i, (v, lat) in enumerate(zip(w.views(band), b.latents)):
        assert np.array_equal(v.cpu().numpy(), lat[3 * i:3 * i + 2]), f"image {i}"


def _check_band_plain(window, band_host, batch):
    for i, (im, lat) in enumerate(zip(window.images, batch.latents)):
        a, nb, first = int(im.band_offset), int(im.band_bytes), int(im.first_stream)
        assert np.array_equal(band_host[a:a + nb], lat.reshape(-1)[first * batch.wss:first * batch.wss + nb]), f"image {i}: band differs"


# ---- through the archive ------------------------------------------------------------------------------------------------------------
SIZES_6 = [(48, 48), (112, 144), (33, 20), (100, 131), (16, 16), (256, 48)]


@pytest.fixture(scope="module")
def archive_of_six(mods, weights):
    _, api, _ = mods
    net = api.RaggedNet(SIZES_6, shared_weights=weights)
    rng = np.random.default_rng(33)
    xin = net.pack([torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in SIZES_6])
    return net.compress_archive(xin, stream_symbols=1024)


def test_rois_through_the_archive(mods, weights, archive_of_six):
    _, api, _ = mods
    b = archive_of_six
    sel = [1, 3]
    net = api.RaggedNet([SIZES_6[i] for i in sel], shared_weights=weights)
    full = net.decompress_archive(b, images=sel)                              # the parent's only way
    torch.cuda.synchronize()
    want = [v.cpu().numpy()[:h, :w] for v, (w, h) in zip(net.views(7, full), net.sizes)]
    for rois in ([(40, 50, 30, 20), (60, 100, 40, 31)], [(0, 0, 1, 1), None], [None, (99, 0, 1, 131)], [None, None]):
        got = net.decompress_archive(b, images=sel, rois=rois)
        torch.cuda.synchronize()
        for v, f, r, size in zip(net.roi_views(got), want, rois, net.sizes):
            x0, y0, w, h = _rect(r, size)
            assert np.array_equal(v.cpu().numpy(), f[y0:y0 + h, x0:x0 + w]), rois
    # the whole archive with rectangles
    net6 = api.RaggedNet(SIZES_6, shared_weights=weights)
    rois6 = [(10, 10, 20, 20), None, (32, 19, 1, 1), (0, 120, 100, 11), (3, 3, 9, 9), (128, 16, 64, 16)]
    full6 = net6.decompress_archive(b)
    got6 = net6.decompress_archive(b, rois=rois6)
    torch.cuda.synchronize()
    for v, f, r, size in zip(net6.roi_views(got6), net6.views(7, full6), rois6, SIZES_6):
        x0, y0, w, h = _rect(r, size)
        assert np.array_equal(v.cpu().numpy(), f.cpu().numpy()[y0:y0 + h, x0:x0 + w])
    # refusals, before any launch
    for bad in ([(0, 0, 1, 1)], [(0, 0, 1, 1)] * 3, [(0, 0, 113, 1), None], [None, (0, 131, 1, 1)], [(5, 5, 0, 1), None], [(1, 2, 3), None]):
        with pytest.raises(ValueError):
            net.decompress_archive(b, images=sel, rois=bad)


def test_roi_decode_is_graph_capturable(mods, weights):
    _, api, _ = mods
    first, fresh = Batch(mods, weights, SIZES_A, 1024, seed=34), Batch(mods, weights, SIZES_A, 1024, seed=35)
    rects = SCENARIOS["cropped-edge"]
    roi = api.RaggedRoi(first.net, rects, coder=first.coder)
    slots, valid = first.slots.clone(), first.enc.clone()
    roi.decode(slots=slots, valid=valid)                                      # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = roi.decode(slots=slots, valid=valid)
    for b in (fresh, first):                                                  # two replays, on other containers each
        slots.copy_(b.slots)
        valid.copy_(b.enc)
        out.fill_(PATTERN)
        roi.status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert not roi.status[:, 0].any()
        for i, (v, full, r, size) in enumerate(zip(roi.views(out), b.recons, rects, SIZES_A)):
            x0, y0, w, h = _rect(r, size)
            assert np.array_equal(v.cpu().numpy(), full[y0:y0 + h, x0:x0 + w]), f"image {i}"


def test_stays_inside_its_buffers(mods, batch_a):
    _lib, api, _ = mods
    L = _lib.lib()
    b = batch_a[1024]
    roi = api.RaggedRoi(b.net, SCENARIOS["interior"], coder=b.coder)
    win = roi.window
    ws_bytes = int(L.sicn_ragged_window_workspace_bytes(win._h))
    assert ws_bytes == int(L.sicn_ragged_coder_workspace_bytes(b.coder._h))
    guarded = lambda nbytes: torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    band, ws, status = guarded(win.band_bytes), guarded(ws_bytes), guarded(4 * 8)
    wlat, pixels = guarded(roi.latent_cut.dst_bytes), guarded(roi.pixel_cut.dst_bytes)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    inner = lambda t, nbytes: t[GUARD:GUARD + nbytes]

    def untouched(t, nbytes):
        h = t.cpu().numpy()
        return (h[:GUARD] == PATTERN).all() and (h[GUARD + nbytes:] == PATTERN).all()

    call = L.sicn_ragged_window_decode_async
    args = (win._h, ptr(b.slots), ptr(b.enc), ptr(band, GUARD), ptr(status, GUARD), ptr(ws, GUARD))
    assert call(*args, ws_bytes - 1, stream) == ENOSPC                         # nothing enqueued
    torch.cuda.synchronize()
    for t in (band, ws, status):
        assert (t.cpu().numpy() == PATTERN).all()
    assert call(*args, ws_bytes, stream) == 0
    roi.latent_cut.run(inner(band, win.band_bytes), inner(wlat, roi.latent_cut.dst_bytes))
    recon, _ = roi.window_net.run_layers(4, 7, inner(wlat, roi.latent_cut.dst_bytes))
    roi.pixel_cut.run(recon, inner(pixels, roi.pixel_cut.dst_bytes))
    torch.cuda.synchronize()
    assert untouched(band, win.band_bytes) and untouched(ws, ws_bytes) and untouched(status, 32)
    assert untouched(wlat, roi.latent_cut.dst_bytes) and untouched(pixels, roi.pixel_cut.dst_bytes)
    st = inner(status, 32).cpu().numpy().view(np.int32).reshape(4, 2)
    assert not st[:, 0].any() and st[:, 1].tolist() == [int(im.band_bytes) for im in win.images[:4]]
    # inside the band tensor, the padding between the bands stays as it was
    h = inner(band, win.band_bytes).cpu().numpy()
    for im, nxt in zip(win.images[:4], list(win.images[1:4]) + [None]):
        end = int(im.band_offset) + int(im.band_bytes)
        assert (h[end:(int(nxt.band_offset) if nxt is not None else win.band_bytes)] == PATTERN).all()
    for v, full, (x0, y0, w, hh) in zip(roi.views(inner(pixels, roi.pixel_cut.dst_bytes)), b.recons, SCENARIOS["interior"]):
        assert np.array_equal(v.cpu().numpy(), full[y0:y0 + hh, x0:x0 + w])


# ---- verdicts -----------------------------------------------------------------------------------------------------------------------
def _container(b, i):
    im = b.coder.images[i]
    return int(im.slot_offset), int(im.n_streams), b.slots[int(im.slot_offset):int(im.slot_offset) + int(b.enc[i, 1])].cpu().numpy()


def _stream_start(b, i, st):
    """Byte offset, inside the slot buffer, of the middle of stream `st` of container i."""
    at, ns, c = _container(b, i)
    table = c[48 + 256:48 + 256 + 4 * ns].view(np.uint32)
    return at + 48 + 256 + 4 * ns + int(table[:st].sum()) + int(table[st]) // 2


def test_a_damaged_stream_matters_only_inside_the_window(mods, batch_a):
    _, api, _ = mods
    b = batch_a[1024]
    rects = [(40, 100, 30, 20), (33, 41, 20, 30), (5, 5, 4, 4), (100, 10, 50, 20)]
    roi = api.RaggedRoi(b.net, rects, coder=b.coder)
    first, end = int(roi.window.images[0].first_stream), int(roi.window.images[0].end_stream)
    assert 0 < first and end <= 12 and first >= 2                             # image 0: rows 5 .. 8 of 9, streams 6 .. 11

    def run(slots):
        out = roi.decode(slots=slots, valid=b.enc)
        torch.cuda.synchronize()
        return roi.status[:, 0].cpu().tolist(), [v.cpu().numpy() for v in roi.views(out)]

    def exact(views, which):
        for i in which:
            x0, y0, w, h = rects[i]
            assert np.array_equal(views[i], b.recons[i][y0:y0 + h, x0:x0 + w]), f"image {i}"

    # outside the window: not read, not reported — and the full decoder does report it
    slots = b.slots.clone()
    slots[_stream_start(b, 0, 1)] ^= 0x5A
    st, views = run(slots)
    assert st == [0, 0, 0, 0]
    exact(views, range(4))
    band = torch.empty(b.coder.latent_bytes, dtype=torch.uint8, device="cuda")
    b.coder.decode(band, slots=slots, valid=b.enc)
    torch.cuda.synchronize()
    assert b.coder.dec_status[0, 0].item() != 0
    # inside: bit 5 for that image alone, the neighbours exact
    slots = b.slots.clone()
    slots[_stream_start(b, 0, first + 1)] ^= 0x5A
    st, views = run(slots)
    assert st == [32, 0, 0, 0]
    exact(views, (1, 2, 3))
    st, views = run(b.slots)                                                  # and the undamaged slots still decode
    assert st == [0, 0, 0, 0]
    exact(views, range(4))


def _patches(ns):
    table = 48 + 256
    yield "magic", 0, 0x4C434954
    yield "version-mode", 4, 1 | (2 << 16)
    yield "image-width (no error)", 8, 7
    yield "image-height (no error)", 12, 7
    for k, name in ((16, "lat_w"), (20, "lat_h"), (24, "lat_c"), (28, "n_symbols"), (32, "n_streams"), (36, "stream_symbols")):
        yield name, k, "+1"
    yield "payload-field + 2", 40, "+2"
    yield "payload-field - 2", 40, "-2"
    yield "payload-field huge", 40, 0x7FFFFFF0
    yield "checksum (bit 7 in the full decoder, nothing here)", 44, "+1"
    yield "frequency table", 48 + 6, "+1"
    yield "length entry above the cap", table + 4 * 3, 2 * 1024 + 256 + 2
    yield "length entry + 2", table + 4 * 2, "+2"
    yield "length entry - 2", table + 4 * (ns - 1), "-2"
    yield "length entry odd", table + 4 * 5, "+1"
    yield "length entry 0", table, 0


def test_patched_fixed_parts_give_the_full_decoders_status_without_bit_7(mods, batch_a):
    """Image 1 of batch A, every stream selected (a full-height window), the container's fixed part patched field by field: the
    window decoder reports what the full decoder reports, bit 7 masked; the other images stay exact."""
    b = batch_a[1024]
    win = b.coder.window([(0, h) for h, _ in b.coder.shapes])
    at, ns, c = _container(b, 1)
    band = torch.empty(win.band_bytes, dtype=torch.uint8, device="cuda")
    full = torch.empty(b.coder.latent_bytes, dtype=torch.uint8, device="cuda")
    seen = set()
    for name, off, value in _patches(ns):
        old = int(c[off:off + 4].view(np.uint32)[0])
        new = (old + int(value)) & 0xFFFFFFFF if isinstance(value, str) else value
        slots = b.slots.clone()
        slots[at + off:at + off + 4] = torch.from_numpy(np.array([new], np.uint32).view(np.uint8).copy()).cuda()
        b.coder.decode(full, slots=slots, valid=b.enc)
        band.fill_(PATTERN)
        win.decode(band, slots=slots, valid=b.enc)
        torch.cuda.synchronize()
        want = b.coder.dec_status[:, 0].cpu().numpy().astype(np.int64)
        got = win.status.cpu().numpy().astype(np.int64)
        assert got[:, 0].tolist() == (want & ~128).tolist(), f"{name}: window {got[:, 0]}, full decoder {want}"
        assert got[0, 0] == got[2, 0] == got[3, 0] == 0, name
        assert got[:, 1].tolist() == [int(im.band_bytes) for im in win.images[:4]], name
        host = band.cpu().numpy()
        for i in (0, 2, 3):
            a = int(win.images[i].band_offset)
            assert np.array_equal(host[a:a + b.latents[i].size], b.latents[i].reshape(-1)), f"{name}: image {i} changed beside a bad container"
        seen.add(int(want[1]))
    assert {0, 128} <= seen and any(s & 4 for s in seen) and any(s & 8 for s in seen) and any(s & 16 for s in seen)
    assert any(s & 32 for s in seen) and any(s & 64 for s in seen)            # every bit of the fixed part was provoked


def test_valid_shorter_than_the_fixed_part(mods, batch_a):
    b = batch_a[1024]
    win = b.coder.window([(2, 3), (0, 9), (0, 1), (1, 2)])
    short = b.enc.clone()
    short[1, 1] = 48 + 256 + 4 * 12 - 1
    band = torch.full((win.band_bytes,), PATTERN, dtype=torch.uint8, device="cuda")
    full = torch.empty(b.coder.latent_bytes, dtype=torch.uint8, device="cuda")
    win.decode(band, slots=b.slots, valid=short)
    b.coder.decode(full, slots=b.slots, valid=short)
    torch.cuda.synchronize()
    st = win.status[:, 0].cpu().tolist()
    assert st[1] & 0x104 == 0x104 and st == b.coder.dec_status[:, 0].cpu().tolist()
    assert [st[0], st[2], st[3]] == [0, 0, 0]
    host = band.cpu().numpy()
    a = int(win.images[1].band_offset)
    assert (host[a:a + int(win.images[1].band_bytes)] == PATTERN).all()       # the refused slot wrote nothing
    for i in (0, 2, 3):
        im = win.images[i]
        lo = int(im.first_stream) * 1024
        assert np.array_equal(host[int(im.band_offset):int(im.band_offset) + int(im.band_bytes)],
                              b.latents[i].reshape(-1)[lo:lo + int(im.band_bytes)])


def test_window_create_refuses_a_bad_second_image_and_leaves_no_handle(mods):
    """sicn_ragged_window_create over a live coder of two images (latents 1 x 1 and 3 x 2, 4 channels): a row range the SECOND image
    cannot hold is refused after the first image's entries were made — SICN_EINVAL and a null handle — and the same coder then
    makes a window of sound rows."""
    _lib, _, _ = mods
    L = _lib.lib()
    u32 = ctypes.c_uint32 * 2
    coder, win = ctypes.c_void_p(), ctypes.c_void_p(1)
    assert L.sicn_ragged_coder_create(u32(1, 3), u32(1, 2), 4, u32(1024, 1024), None, None, 2, ctypes.byref(coder)) == 0
    try:
        for r0, rh in [((0, 0), (1, 0)), ((0, 2), (1, 1)), ((0, 1), (1, 2))]:       # no rows; behind the latent; past its end
            win.value = 1
            assert L.sicn_ragged_window_create(coder, u32(*r0), u32(*rh), ctypes.byref(win)) == -22
            assert not win.value
        assert L.sicn_ragged_window_create(coder, u32(0, 1), u32(1, 1), ctypes.byref(win)) == 0 and win.value
        assert L.sicn_ragged_window_workspace_bytes(win) == L.sicn_ragged_coder_workspace_bytes(coder)
        L.sicn_ragged_window_free(win)
    finally:
        L.sicn_ragged_coder_free(coder)
