"""GPU checks of the moving ROI decode (include/sicn_ragged_roi_move.h, csrc/k_ragged_roi_move.hip; run with -m gpu on an MI355X):
pixel rectangles of fixed size whose positions are read from device memory on every call.  Byte equality throughout; the reference
is the full decode of the same containers — RaggedLatentCoder.decode and layers 4-7, or decompress_archive(images=) — sliced in
numpy, computed once per batch and never changed."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 4096
PATTERN = 0xA5
LAT_C = 192
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
SIZES = [(112, 144), (100, 131), (16, 16), (256, 48), (64, 400)]       # (width, height): latents 7 x 9, 7 x 9, 1 x 1, 16 x 3, 4 x 25
# (image, w, h): 1 x 1, 16 x 16, 20 x 20, 33 x 15, full width, full height, the image whole; three slots of image 0, two of 1, 2, 3
# and 4; the images in no order
SLOTS = [(4, 64, 400), (3, 256, 15), (3, 33, 15), (1, 20, 131), (2, 16, 16), (0, 20, 20), (0, 1, 1), (2, 1, 1), (0, 16, 16), (4, 33, 15),
         (1, 100, 131)]


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
        for a in self.latents + self.recons:
            a.setflags(write=False)
        self.enc = self.coder.enc_status.clone()
        self.slots = self.coder.slot_buffer.clone()                  # pristine copies for the tests that damage a container


@pytest.fixture(scope="module")
def batches(mods, weights):
    return {wss: Batch(mods, weights, SIZES, wss, seed=41) for wss in (1024, 16384)}


def _clamp(batch, slots, xy):
    return [(min(max(int(x), 0), batch.sizes[i][0] - w), min(max(int(y), 0), batch.sizes[i][1] - h)) for (i, w, h), (x, y) in zip(slots, xy)]


def _check_pixels(mv, batch, xy, out, which=None):
    """The ROI pixels against the sliced full decode, at the clamped positions."""
    views = mv.views(out)
    for k, ((i, w, h), (x, y)) in enumerate(zip(mv.slots, _clamp(batch, mv.slots, xy))):
        if which is not None and k not in which:
            continue
        got = views[k].cpu().numpy()
        assert got.shape == (h, w, 3)
        assert np.array_equal(got, batch.recons[i][y:y + h, x:x + w]), f"slot {k} {mv.slots[k]} at {(x, y)}: ROI pixels differ from the full decode"


def _selection_of(mv, batch, k, x, y):
    """(first_stream, end_stream, symbols, r0, c0) of slot k placed at (x, y), in plain arithmetic on the host's placement."""
    from simple_image_compression_network_amd import _lib
    (i, w, h), s = mv.slots[k], mv.layout[k]
    lh, lw = batch.coder.shapes[i]
    p = _lib.RaggedRoiPlaced()
    assert _lib.lib().sicn_ragged_roi_move_place(4, batch.sizes[i][0], batch.sizes[i][1], lw, lh, w, h, int(x), int(y), ctypes.byref(p)) == 0
    R, n, wss = lw * LAT_C, lw * lh * LAT_C, batch.wss
    first, end = p.r0 * R // wss, -(-(p.r0 + int(s.rh_cap)) * R // wss)
    return first, end, min(n, end * wss) - first * wss, int(p.r0), int(p.c0)


def _selection(mv, batch, xy):
    return [_selection_of(mv, batch, k, x, y) for k, (x, y) in enumerate(xy)]


def _guarded(mv):
    """Every buffer of the object replaced by the inside of a larger one filled with the pattern; returns the larger ones."""
    outer = {}
    for name in ("band", "latent", "recon", "roi", "ws", "status", "flags"):
        t = getattr(mv, name)
        raw = t.view(-1).view(torch.uint8)
        big = torch.full((GUARD + raw.numel() + GUARD,), PATTERN, dtype=torch.uint8, device=t.device)
        inner = big[GUARD:GUARD + raw.numel()]
        inner.copy_(raw)
        setattr(mv, name, inner if t.dtype == torch.uint8 else inner.view(torch.int32).view(t.shape))
        outer[name] = (big, raw.numel())
    return outer


def _guards_untouched(outer):
    for name, (big, n) in outer.items():
        h = big.cpu().numpy()
        assert (h[:GUARD] == PATTERN).all() and (h[GUARD + n:] == PATTERN).all(), f"{name}: written outside the buffer"


def _position_sets(mv, batch, count, seed):
    """`count` position sets: the four corners, two edges, then seeded interior positions; the last two sets hold, per slot, a
    position whose selection has max_streams streams and one that has one stream fewer (where the slot has such positions)."""
    rng = np.random.default_rng(seed)
    last = [(batch.sizes[i][0] - w, batch.sizes[i][1] - h) for i, w, h in mv.slots]
    sets = [[(0, 0)] * len(last), list(last), [(a, 0) for a, _ in last], [(0, b) for _, b in last], [(a // 2, 0) for a, _ in last],
            [(0, b // 2) for _, b in last]]
    while len(sets) < count - 2:
        sets.append([(int(rng.integers(0, a + 1)), int(rng.integers(0, b + 1))) for a, b in last])
    most, fewer = [], []
    for k, (a, b) in enumerate(last):
        cand = {}
        for y in range(b + 1):
            first, end, *_ = _selection_of(mv, batch, k, 0, y)
            cand[y] = end - first
        ms = int(mv.layout[k].max_streams)
        assert max(cand.values()) == ms, f"slot {k}: no position selects max_streams"
        most.append((a // 3, next(y for y, c in cand.items() if c == ms)))
        fewer.append((a // 3, next((y for y, c in cand.items() if c == ms - 1), b // 2)))
    return sets + [most, fewer], most, fewer


def test_streams_of_the_batch_are_what_the_issue_counts(mods, batches):
    assert [int(im.n_streams) for im in batches[1024].coder.images[:5]] == [12, 12, 1, 9, 19]
    assert [int(im.n_streams) for im in batches[16384].coder.images[:5]] == [1, 1, 1, 1, 2]
    mv = batches[1024].net.moving_roi([(0, 20, 20)], coder=batches[1024].coder)
    assert int(mv.layout[0].max_streams) == 8 and mv.items == 8                # at most 8 of 12


@pytest.mark.parametrize("wss", [1024, 16384])
def test_one_object_twelve_positions_stage_by_stage(mods, batches, wss):
    """One MovingRoi over eleven slots — every slot size of the issue, two and three slots on one image, images in no order — and
    twelve position sets.  Every buffer has guard bands; before each call the band is filled with a pattern and the workspace
    dirtied with another byte: every band byte outside this call's selected symbols stays the pattern (surplus work items write
    nothing), and what an earlier call left in the workspace changes nothing."""
    b = batches[wss]
    mv = b.net.moving_roi(SLOTS, coder=b.coder)
    outer = _guarded(mv)
    sets, most, fewer = _position_sets(mv, b, 12, seed=wss)
    assert len(sets) == 12
    if wss == 1024:
        sel_most, sel_fewer = _selection(mv, b, most), _selection(mv, b, fewer)
        surplus = [int(s.max_streams) - (e - f) for s, (f, e, *_) in zip(mv.layout, sel_fewer)]
        assert sum(1 for v in surplus if v == 1) >= 4, "slots with a position one stream below their capacity"
        assert all(int(s.max_streams) == e - f for s, (f, e, *_) in zip(mv.layout, sel_most))
        assert any(int(s.max_streams) < int(b.coder.images[i].n_streams) for (i, _, _), s in zip(SLOTS, mv.layout))
    for k, xy in enumerate(sets):
        mv.band.fill_(PATTERN)
        mv.ws.fill_((k * 37 + 11) & 255)
        out = mv.decode(xy)
        torch.cuda.synchronize()
        st = mv.status.cpu().numpy().astype(np.int64)
        sel = _selection(mv, b, xy)
        assert not st[:, 0].any(), (k, st)
        assert st[:, 1].tolist() == [s[2] for s in sel], k
        assert not mv.flags.cpu().numpy().any(), k
        # 1: the band — the selected symbols are the full latent's, every other byte is the pattern
        band = mv.band.cpu().numpy()
        at = 0
        for j, ((i, _, _), s, (first, end, symbols, _, _)) in enumerate(zip(SLOTS, mv.layout, sel)):
            a = int(s.band_offset)
            assert np.array_equal(band[a:a + symbols], b.latents[i].reshape(-1)[first * wss:first * wss + symbols]), f"set {k} slot {j}: band"
            assert (band[at:a] == PATTERN).all(), f"set {k}: bytes in front of band {j} were written"
            at = a + symbols
        assert (band[at:] == PATTERN).all(), f"set {k}: bytes behind the last band were written"
        # 2: the window latents
        lat = mv.latent.cpu().numpy()
        for j, ((i, _, _), s, (_, _, _, r0, c0)) in enumerate(zip(SLOTS, mv.layout, sel)):
            rh, cw = int(s.rh_cap), int(s.cw_cap)
            got = lat[int(s.latent_offset):int(s.latent_offset) + rh * cw * LAT_C].reshape(rh, cw, LAT_C)
            assert np.array_equal(got, b.latents[i][r0:r0 + rh, c0:c0 + cw]), f"set {k} slot {j}: window latent"
        # 3: the ROI pixels
        _check_pixels(mv, b, xy, out)
    _guards_untouched(outer)


def test_uniform_slots_come_back_as_one_array(mods, batches):
    b = batches[1024]
    mv = b.net.moving_roi([(0, 33, 15), (3, 33, 15), (0, 33, 15), (1, 33, 15)], coder=b.coder)
    xy = [(5, 100), (200, 30), (79, 0), (0, 116)]
    out = mv.decode(xy)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (4, 15, 33, 3) and out.data_ptr() == mv.roi.data_ptr()
    for got, (i, w, h), (x, y) in zip(out.cpu().numpy(), mv.slots, xy):
        assert np.array_equal(got, b.recons[i][y:y + h, x:x + w])
    own = torch.full((mv.roi_bytes,), PATTERN, dtype=torch.uint8, device="cuda")
    again = mv.decode(torch.tensor(xy, dtype=torch.int32, device="cuda"), out=own)
    torch.cuda.synchronize()
    assert again.data_ptr() == own.data_ptr() and torch.equal(again, out)
    for bad in ([(0, 0)] * 3, torch.zeros((4, 2), dtype=torch.int64, device="cuda"), torch.zeros((2, 4), dtype=torch.int32, device="cuda")):
        with pytest.raises((ValueError, TypeError)):
            mv.decode(bad)
    for bad in ([], [(5, 20, 20)], [(0, 113, 20)], [(0, 20, 145)], [(0, 0, 20)], [(0, 20)]):
        with pytest.raises(ValueError):
            b.net.moving_roi(bad, coder=b.coder)


@pytest.mark.parametrize("wss", [1024, 16384])
def test_clamped_positions(mods, batches, wss):
    _lib, _, _ = mods
    b = batches[wss]
    mv = b.net.moving_roi(SLOTS, coder=b.coder)
    rng = np.random.default_rng(5)
    inside = [(int(rng.integers(0, b.sizes[i][0] - w + 1)), int(rng.integers(0, b.sizes[i][1] - h + 1))) for i, w, h in SLOTS]
    outside = [(-1, 5), (INT32_MAX, 3), (7, -9), (INT32_MIN, INT32_MIN), (0, 1), (93, 125), (112, 144), (3, INT32_MAX), (-5, INT32_MAX),
               (INT32_MIN, 386), (1, 0)]
    for pick in (range(0, 11, 2), range(1, 11, 2), range(11)):
        xy = [outside[k] if k in pick else inside[k] for k in range(11)]
        want = [int(c != (x, y)) for c, (x, y) in zip(_clamp(b, SLOTS, xy), xy)]
        assert sum(want) >= 4 and (len(pick) == 11 or sum(want) <= 6)
        out = mv.decode(torch.tensor(xy, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        assert mv.flags.cpu().tolist() == want == [p["flags"] for p in mv.place(xy)]
        assert not mv.status[:, 0].any()
        _check_pixels(mv, b, xy, out)                                        # the clamped rectangles, and the other slots unaffected


@pytest.mark.parametrize("wss", [1024, 16384])
def test_equal_to_ragged_roi_with_one_slot_per_image(mods, batches, wss):
    _, api, _ = mods
    b = batches[wss]
    slots = [(0, 20, 20), (1, 33, 15), (2, 16, 16), (3, 256, 15), (4, 17, 400)]
    mv = b.net.moving_roi(slots, coder=b.coder)
    for xy in ([(40, 50), (33, 41), (0, 0), (0, 20), (30, 0)], [(92, 124), (67, 116), (0, 0), (0, 33), (47, 0)], [(0, 0)] * 5):
        rects = [(x, y, w, h) for (_, w, h), (x, y) in zip(slots, xy)]
        roi = api.RaggedRoi(b.net, rects, coder=b.coder)
        want = roi.decode()
        got = mv.decode(xy)
        torch.cuda.synchronize()
        assert torch.equal(got.reshape(-1), want)
        assert not mv.status[:, 0].any() and not roi.status[:, 0].any()


# ---- both forms of the decode kernel --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch_big(mods, weights):
    return Batch(mods, weights, [(640, 400)] * 8, 1024, seed=42)


def test_tall_slots_run_the_two_table_form(mods, batch_big):
    b = batch_big
    slots = [(i, 20 + i, 300) for i in range(8)]
    mv = b.net.moving_roi(slots, coder=b.coder)
    assert mv.items == 8 * 174 == 1392 > 5 * 256                              # above 5 x n_cu on a whole chip: k_roi_move_decode<false>
    for xy in ([(300 + 7 * i, 11 * i) for i in range(8)], [(0, 100), (600, 0), (17, 5), (320, 99), (1, 1), (500, 50), (30, 100), (90, 37)]):
        mv.band.fill_(PATTERN)
        out = mv.decode(xy)
        torch.cuda.synchronize()
        sel = _selection(mv, b, xy)
        assert not mv.status[:, 0].any() and mv.status[:, 1].cpu().tolist() == [s[2] for s in sel]
        assert any(e - f < 174 for f, e, *_ in sel)                           # surplus items ran
        band = mv.band.cpu().numpy()
        for (i, _, _), s, (first, end, symbols, _, _) in zip(slots, mv.layout, sel):
            a = int(s.band_offset)
            assert np.array_equal(band[a:a + symbols], b.latents[i].reshape(-1)[first * 1024:first * 1024 + symbols])
            assert (band[a + symbols:a + 174 * 1024] == PATTERN).all()
        _check_pixels(mv, b, xy, out)


def test_short_slots_run_the_one_table_form(mods, batch_big):
    b = batch_big
    mv = b.net.moving_roi([(i, 64, 20) for i in range(8)], coder=b.coder)
    assert mv.items == 8 * 39 < 5 * 256                                       # k_roi_move_decode<true>
    xy = [(70 * i, 50 * i) for i in range(8)]
    out = mv.decode(xy)
    torch.cuda.synchronize()
    assert not mv.status[:, 0].any()
    _check_pixels(mv, b, xy, out)


# ---- verdicts -----------------------------------------------------------------------------------------------------------------------
def _container(b, i):
    im = b.coder.images[i]
    return int(im.slot_offset), int(im.n_streams), b.slots[int(im.slot_offset):int(im.slot_offset) + int(b.enc[i, 1])].cpu().numpy()


def _stream_middle(b, i, st):
    """Byte offset, inside the slot buffer, of the middle of stream `st` of container i."""
    at, ns, c = _container(b, i)
    table = c[48 + 256:48 + 256 + 4 * ns].view(np.uint32)
    return at + 48 + 256 + 4 * ns + int(table[:st].sum()) + int(table[st]) // 2


def test_a_damaged_stream_is_reported_by_the_slot_that_moves_onto_it(mods, batches):
    b = batches[1024]
    slots = [(0, 20, 20), (1, 33, 15), (0, 20, 20), (3, 33, 15)]
    mv = b.net.moving_roi(slots, coder=b.coder)
    damaged = b.slots.clone()
    damaged[_stream_middle(b, 0, 1)] ^= 0x5A                                   # stream 1 of image 0: latent row 0 and 1
    away = [(40, 124), (33, 41), (60, 124), (100, 10)]                         # both slots of image 0 on its last rows
    onto = [(40, 0), (33, 41), (60, 124), (100, 10)]                           # slot 0 moved to the top
    assert _selection(mv, b, away)[0][0] > 1 and _selection(mv, b, away)[2][0] > 1
    first, end, *_ = _selection(mv, b, onto)[0]
    assert first <= 1 < end

    def run(xy, slot_buffer):
        out = mv.decode(xy, slots=slot_buffer, valid=b.enc)
        torch.cuda.synchronize()
        return mv.status[:, 0].cpu().tolist(), out

    st, out = run(away, damaged)                                               # outside every window: not read, not reported
    assert st == [0, 0, 0, 0]
    _check_pixels(mv, b, away, out)
    full = torch.empty(b.coder.latent_bytes, dtype=torch.uint8, device="cuda")
    b.coder.decode(full, slots=damaged, valid=b.enc)
    torch.cuda.synchronize()
    assert b.coder.dec_status[0, 0].item() != 0                                # ... and the full decoder does report it
    st, out = run(onto, damaged)                                               # moved onto it: that slot alone
    assert st == [32, 0, 0, 0]
    _check_pixels(mv, b, onto, out, which=(1, 2, 3))                           # the second slot of the same image stays clean and exact
    st, out = run(onto, b.slots)                                               # and the undamaged slots still decode
    assert st == [0, 0, 0, 0]
    _check_pixels(mv, b, onto, out)


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


def test_patched_fixed_parts_give_the_full_decoders_status_without_bit_7(mods, batches):
    """Image 1 whole in slot 1 — every stream selected — and in slot 3 a small rectangle of it; its container's fixed part patched
    field by field: slot 1 reports what the full decoder reports, bit 7 masked, slot 3 the same but for what only a selected
    stream can say (bit 5 of a stream outside its window); the slots of other images stay clean and exact."""
    b = batches[1024]
    slots = [(0, 20, 20), (1, 100, 131), (3, 33, 15), (1, 1, 1), (2, 16, 16)]
    xy = [(40, 50), (0, 0), (100, 10), (50, 130), (0, 0)]
    mv = b.net.moving_roi(slots, coder=b.coder)
    at, ns, c = _container(b, 1)
    full = torch.empty(b.coder.latent_bytes, dtype=torch.uint8, device="cuda")
    seen = set()
    for name, off, value in _patches(ns):
        old = int(c[off:off + 4].view(np.uint32)[0])
        new = (old + int(value)) & 0xFFFFFFFF if isinstance(value, str) else value
        damaged = b.slots.clone()
        damaged[at + off:at + off + 4] = torch.from_numpy(np.array([new], np.uint32).view(np.uint8).copy()).cuda()
        b.coder.decode(full, slots=damaged, valid=b.enc)
        out = mv.decode(xy, slots=damaged, valid=b.enc)
        torch.cuda.synchronize()
        want = int(b.coder.dec_status[1, 0].item())
        got = mv.status.cpu().numpy().astype(np.int64)
        assert got[1, 0] == want & ~128, f"{name}: slot {got[1, 0]}, full decoder {want}"
        assert got[3, 0] & ~32 == want & ~(128 | 32), f"{name}: the small slot {got[3, 0]}, full decoder {want}"
        assert got[0, 0] == got[2, 0] == got[4, 0] == 0, name
        assert got[:, 1].tolist() == [s[2] for s in _selection(mv, b, xy)], name
        _check_pixels(mv, b, xy, out, which=(0, 2, 4))
        seen.add(want)
    assert {0, 128} <= seen and any(s & 4 for s in seen) and any(s & 8 for s in seen) and any(s & 16 for s in seen)
    assert any(s & 32 for s in seen) and any(s & 64 for s in seen)            # every bit of the fixed part was provoked


def test_valid_shorter_than_the_fixed_part(mods, batches):
    b = batches[1024]
    slots = [(0, 20, 20), (1, 100, 131), (3, 33, 15), (1, 1, 1)]
    xy = [(40, 50), (0, 0), (100, 10), (50, 130)]
    mv = b.net.moving_roi(slots, coder=b.coder)
    short = b.enc.clone()
    short[1, 1] = 48 + 256 + 4 * 12 - 1
    full = torch.empty(b.coder.latent_bytes, dtype=torch.uint8, device="cuda")
    mv.band.fill_(PATTERN)
    out = mv.decode(xy, slots=b.slots, valid=short)
    b.coder.decode(full, slots=b.slots, valid=short)
    torch.cuda.synchronize()
    st = mv.status[:, 0].cpu().tolist()
    want = b.coder.dec_status[:, 0].cpu().tolist()
    assert want[1] & 0x104 == 0x104 and st == [0, want[1], 0, want[1]]
    band = mv.band.cpu().numpy()
    for k in (1, 3):                                                           # the refused slot wrote nothing
        a = int(mv.layout[k].band_offset)
        assert (band[a:a + int(mv.layout[k].max_streams) * 1024] == PATTERN).all()
    _check_pixels(mv, b, xy, out, which=(0, 2))


# ---- graph, archive, memory ---------------------------------------------------------------------------------------------------------
def test_a_captured_chain_replays_with_new_positions(mods, batches):
    b = batches[1024]
    slots = [(4, 33, 15), (0, 20, 20), (3, 33, 15), (0, 16, 16), (1, 20, 131)]
    mv = b.net.moving_roi(slots, coder=b.coder)
    last = torch.tensor([[b.sizes[i][0] - w, b.sizes[i][1] - h] for i, w, h in slots], dtype=torch.int32, device="cuda")
    xy = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    mv.decode(xy)                                                              # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = mv.decode(xy)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    drawn = (torch.rand((5, 2), device="cuda", generator=gen) * (last + 1).float()).to(torch.int32).clamp_(max=last)   # on the device
    for new in (last, drawn, torch.tensor([[10, 380], [-3, 60], [200, 33], [50, 50], [80, 0]], dtype=torch.int32, device="cuda")):
        xy.copy_(new)
        out.fill_(PATTERN)
        mv.status.fill_(-1)
        mv.flags.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        host = xy.cpu().tolist()
        assert not mv.status[:, 0].any()
        assert mv.flags.cpu().tolist() == [int(c != tuple(p)) for c, p in zip(_clamp(b, slots, host), host)]
        _check_pixels(mv, b, host, out)


def test_an_archive_unpacked_once_serves_many_moves(mods, weights):
    _, api, codec = mods
    sizes6 = [(48, 48), (112, 144), (33, 20), (100, 131), (16, 16), (256, 48)]
    net6 = api.RaggedNet(sizes6, shared_weights=weights)
    rng = np.random.default_rng(43)
    xin = net6.pack([torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in sizes6])
    blob = net6.compress_archive(xin, stream_symbols=1024)
    sel = [1, 3, 5]
    net = api.RaggedNet([sizes6[i] for i in sel], shared_weights=weights)
    full = net.decompress_archive(blob, images=sel)                            # the full decode of the same containers
    torch.cuda.synchronize()
    want = [v.cpu().numpy()[:h, :w] for v, (w, h) in zip(net.views(7, full), net.sizes)]
    coder = net.latent_coder(1024)
    archive = codec.RaggedArchive([coder])
    valid, = archive.unpack(blob, images=sel)                                  # once
    slots = [(2, 64, 16), (0, 20, 20), (1, 33, 15), (0, 20, 20)]
    mv = net.moving_roi(slots, coder=coder)
    for xy in ([(0, 0)] * 4, [(192, 32), (92, 124), (67, 116), (0, 124)], [(100, 7), (41, 77), (13, 60), (55, 3)], [(31, 15), (16, 16), (32, 32), (17, 31)]):
        out = mv.decode(xy, valid=valid)
        torch.cuda.synchronize()
        assert not mv.status[:, 0].any()
        for v, (i, w, h), (x, y) in zip(mv.views(out), slots, xy):
            assert np.array_equal(v.cpu().numpy(), want[i][y:y + h, x:x + w]), (xy, i)
    archive.check()


def test_decode_allocates_nothing(mods, batches):
    b = batches[1024]
    mv = b.net.moving_roi(SLOTS, coder=b.coder)
    xy_dev = torch.zeros((len(SLOTS), 2), dtype=torch.int32, device="cuda")
    host = [(1, 2)] * len(SLOTS)
    mv.decode(xy_dev)                                                          # the first call
    torch.cuda.synchronize()
    for xy in (xy_dev, host, xy_dev, host):
        before = torch.cuda.memory_allocated()
        out = mv.decode(xy)
        after = torch.cuda.memory_allocated()
        torch.cuda.synchronize()
        assert after == before == torch.cuda.memory_allocated()
        assert out.data_ptr() == mv.roi.data_ptr()
    _check_pixels(mv, b, host, out)


def test_argument_checks_come_before_any_launch(mods, batches):
    _lib, _, _ = mods
    L = _lib.lib()
    b = batches[1024]
    mv = b.net.moving_roi(SLOTS, coder=b.coder)
    outer = _guarded(mv)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    xy = torch.zeros((len(SLOTS), 2), dtype=torch.int32, device="cuda")
    need = int(L.sicn_ragged_roi_move_workspace_bytes(mv._h))
    assert need == mv.ws.numel() > 0
    for name in ("band", "latent", "status", "flags", "ws"):
        getattr(mv, name).view(-1).view(torch.uint8).fill_(PATTERN)
    args = [mv._h, ptr(xy), ptr(b.slots), ptr(b.enc), ptr(mv.band), ptr(mv.latent), ptr(mv.status), ptr(mv.flags), ptr(mv.ws)]
    call = L.sicn_ragged_roi_move_decode_async
    assert call(*args, need - 1, stream) == -28
    assert call(*args[:8], ptr(mv.ws, 8), need, stream) == -22
    assert call(*args[:1], ptr(xy, 2), *args[2:], need, stream) == -22
    assert call(*args[:4], None, *args[5:], need, stream) == -22
    torch.cuda.synchronize()
    for name in ("band", "latent", "status", "flags", "ws"):                   # nothing was enqueued
        assert (getattr(mv, name).view(-1).view(torch.uint8).cpu().numpy() == PATTERN).all(), name
    assert call(*args, need, stream) == 0
    torch.cuda.synchronize()
    _guards_untouched(outer)


def test_create_refuses_a_bad_second_slot_and_leaves_no_handle(mods):
    """sicn_ragged_roi_move_create over a live coder of two images (16 x 16 and 48 x 32: latents 1 x 1 and 3 x 2, 4 channels): a
    SECOND slot its image cannot hold is refused after the first slot was laid out — SICN_EINVAL and a null handle — and the same
    coder then makes an object of sound slots."""
    _lib, _, _ = mods
    L = _lib.lib()
    u32 = ctypes.c_uint32 * 2
    coder, mv = ctypes.c_void_p(), ctypes.c_void_p(1)
    assert L.sicn_ragged_coder_create(u32(1, 3), u32(1, 2), 4, u32(1024, 1024), u32(16, 48), u32(16, 32), 2, ctypes.byref(coder)) == 0
    try:
        for bad in [(1, 49, 20), (1, 20, 0), (2, 16, 16)]:                           # wider than its image; empty; no such image
            mv.value = 1
            slots = (_lib.RaggedRoiSlot * 2)(_lib.RaggedRoiSlot(0, 16, 16), _lib.RaggedRoiSlot(*bad))
            assert L.sicn_ragged_roi_move_create(coder, slots, 2, ctypes.byref(mv)) == -22
            assert not mv.value
        slots = (_lib.RaggedRoiSlot * 2)(_lib.RaggedRoiSlot(0, 16, 16), _lib.RaggedRoiSlot(1, 20, 20))
        assert L.sicn_ragged_roi_move_create(coder, slots, 2, ctypes.byref(mv)) == 0 and mv.value
        assert L.sicn_ragged_roi_move_workspace_bytes(mv) == L.sicn_ragged_coder_workspace_bytes(coder)
        L.sicn_ragged_roi_move_free(mv)
    finally:
        L.sicn_ragged_coder_free(coder)
