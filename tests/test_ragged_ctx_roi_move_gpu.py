"""GPU checks of the hyperprior moving ROI decode (include/sicn_ragged_ctx_roi_move.h, csrc/k_ragged_ctx_roi_move.hip,
hyperprior.MovingHyperpriorRoi; run with -m gpu on an MI355X): pixel rectangles of fixed size whose positions are read from device
memory on every call, decoded from the rANS-WC streams of a ragged hyperprior batch after ONE prepare per set of containers.  Byte
equality throughout; the reference is the codec's own full decode() + main.cropped of the same containers, sliced in numpy, computed
once per configuration and never changed."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 4096
PATTERN = 0xA5
LAT_C = 192
WPB = 8
SEED = 7
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
SIZES = [(592, 592), (160, 640), (48, 48), (100, 36), (16, 16)]       # (width, height): latents 37 x 37, 10 x 40, 3 x 3, 7 x 3, 1 x 1
# (image, w, h): two 20 x 20 slots and a wide one on image 0, a small and a tall one on image 1, an image whole (slot 4), a 1 x 1
# latent without non-anchor capacity (slot 6); the images in no order
SLOTS = [(0, 20, 20), (1, 33, 15), (0, 256, 15), (1, 17, 400), (2, 16, 16), (3, 33, 15), (4, 16, 16), (0, 20, 20)]
HEADER, TABLES = 48, 16 * 256


class World:
    """A ragged hyperprior batch, its containers, and the full path's results on the host — computed once, never changed."""

    def __init__(self, sizes, use_gdn, wss, seed=33):
        from simple_image_compression_network_amd import hyperprior
        self.sizes, self.use_gdn, self.wss = sizes, use_gdn, wss
        rng = np.random.default_rng(seed)
        images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
        self.rc = rc = hyperprior.RaggedHyperpriorCodec(sizes, seed=SEED, use_gdn=use_gdn, y_stream_symbols=wss)
        rc.encode(rc.main.pack([torch.from_numpy(x) for x in images]))
        full = rc.decode()
        rc.check()
        self.recons = [v.cpu().numpy() for v in rc.main.crop_views(rc.main.cropped(full))]
        self.latents = [v.cpu().numpy() for v in rc.main.views(3, rc.y_hat)]          # the full y_hat of the same containers
        for a in self.recons + self.latents:
            a.setflags(write=False)
        self.containers = rc.containers()
        self.lat = [(a.shape[1], a.shape[0]) for a in self.latents]                   # (lat_w, lat_h)
        self._orders = {}

    def order(self, i):
        """Per set, the flat [H][W][C] offset of every symbol of image i in the set's own order: raster over row pairs."""
        if i not in self._orders:
            W, H = self.lat[i]
            ch = np.arange(LAT_C)
            out = []
            for s in (0, 1):
                px = []
                for r in range((H + 1) // 2):
                    px += [(2 * r, x) for x in range(s, W, 2)]
                    if 2 * r + 1 < H:
                        px += [(2 * r + 1, x) for x in range(1 - s, W, 2)]
                out.append((np.array([(y * W + x) * LAT_C for y, x in px], dtype=np.int64).reshape(-1, 1) + ch).reshape(-1))
            self._orders[i] = out
        return self._orders[i]


@pytest.fixture(scope="module")
def worlds():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    made = {}

    def get(use_gdn, wss, sizes=None):
        key = (use_gdn, wss, tuple(sizes or SIZES))
        if key not in made:
            made[key] = World(list(sizes or SIZES), use_gdn, wss)
        return made[key]
    return get


CONFIGS = [pytest.param(True, 1024, id="gdn-1024"), pytest.param(True, 16384, id="gdn-16384"), pytest.param(False, 1024, id="relu-1024"),
           pytest.param(False, 16384, id="relu-16384")]


# ---- the host's placement, per slot ----------------------------------------------------------------------------------------------------
def _place(wd, mv, k, x, y):
    from simple_image_compression_network_amd import _lib
    (i, w, h), s = mv.slots[k], mv.layout[k]
    (lw, lh), (iw, ih) = wd.lat[i], wd.sizes[i]
    p = _lib.RaggedCtxRoiPlaced()
    assert _lib.lib().sicn_ragged_ctx_roi_move_place(iw, ih, lw, lh, LAT_C, wd.wss, w, h, int(x), int(y), int(s.band_offset), ctypes.byref(p)) == 0
    return p


def _clamp(wd, slots, xy):
    return [(min(max(int(x), 0), wd.sizes[i][0] - w), min(max(int(y), 0), wd.sizes[i][1] - h)) for (i, w, h), (x, y) in zip(slots, xy)]


def _expected_band(wd, mv, k, p):
    """What slot k's band must hold after a decode at placement p: the full latent's symbols where a selected stream holds the
    position, ZERO everywhere else, over the whole capacity of the band."""
    i = mv.slots[k][0]
    lw, _ = wd.lat[i]
    R, S = lw * LAT_C, wd.wss
    flat = wd.latents[i].reshape(-1)
    want = np.zeros(flat.size, np.uint8)
    held = 0
    for s in (0, 1):
        idx = wd.order(i)[s][p.first_stream[s] * S:p.end_stream[s] * S]
        want[idx] = flat[idx]
        held += idx.size
    assert held == p.symbols
    rows = want[p.band_row0 * R:(p.band_row0 + p.band_rows) * R]
    assert not want[:p.band_row0 * R].any() and not want[(p.band_row0 + p.band_rows) * R:].any(), "the band's rows hold every selected symbol"
    return np.concatenate([rows, np.zeros((int(mv.layout[k].band_rows_cap) - p.band_rows) * R, np.uint8)])


def _check_pixels(mv, wd, xy, out, which=None):
    """The ROI pixels against the sliced full decode, at the clamped positions."""
    views = mv.views(out)
    for k, ((i, w, h), (x, y)) in enumerate(zip(mv.slots, _clamp(wd, mv.slots, xy))):
        if which is not None and k not in which:
            continue
        got = views[k].cpu().numpy()
        assert got.shape == (h, w, 3)
        assert np.array_equal(got, wd.recons[i][y:y + h, x:x + w]), f"slot {k} {mv.slots[k]} at {(x, y)}: ROI pixels differ from the full decode"


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


def _randomise(mv, gen, coder_ws):
    """Random bytes in every tensor a decode writes; of the workspace only the slots' own blocks (the images' are prepare's)."""
    for t in (mv.band, mv.latent, mv.recon, mv.roi, mv.ws[coder_ws:]):
        t.copy_(torch.randint(0, 256, (t.numel(),), dtype=torch.uint8, device=t.device, generator=gen))
    mv.status.fill_(-1)
    mv.flags.fill_(-1)


def _position_sets(wd, mv, seed):
    """Twelve position sets, chosen per slot from the host's placement: the four corners; positions that select exactly the capacity
    of the anchor streams, of the non-anchor streams and of the band rows; one that leaves a whole work item of a decode grid
    without a stream (where the slot has one); an odd and an even r0 (where the slot has both); two seeded ones.  Returns the sets
    and, per slot, what the scan found."""
    rng = np.random.default_rng(seed)
    n = len(mv.slots)
    last = [(wd.sizes[i][0] - w, wd.sizes[i][1] - h) for i, w, h in mv.slots]
    per_slot, found = [], []
    for k, (a, b) in enumerate(last):
        s = mv.layout[k]
        scan = {y: _place(wd, mv, k, a // 3, y) for y in range(b + 1)}
        sel = lambda p, t: p.end_stream[t] - p.first_stream[t]
        pick = lambda cond, default: next((y for y, p in scan.items() if cond(p)), default)
        cap0 = pick(lambda p: sel(p, 0) == s.max_streams[0], None)
        cap1 = pick(lambda p: sel(p, 1) == s.max_streams[1], None)
        rows = pick(lambda p: p.band_rows == s.band_rows_cap, None)
        assert cap0 is not None and cap1 is not None and rows is not None, f"slot {k}: a capacity no pixel position attains"
        surplus = pick(lambda p: any(-(-sel(p, t) // WPB) < s.items[t] for t in (0, 1)), None)
        odd, even = pick(lambda p: p.px.r0 & 1, None), pick(lambda p: not p.px.r0 & 1, 0)
        ys = [0, b, 0, b, cap0, cap1, rows, b // 2 if surplus is None else surplus, b // 3 if odd is None else odd, even,
              int(rng.integers(0, b + 1)), int(rng.integers(0, b + 1))]
        xs = [0, a, a, 0] + [a // 3] * 6 + [int(rng.integers(0, a + 1)), int(rng.integers(0, a + 1))]
        per_slot.append(list(zip(xs, ys)))
        found.append(dict(surplus=surplus is not None, odd=odd is not None, last_r0=scan[b].px.r0))
    return [[per_slot[k][j] for k in range(n)] for j in range(12)], found


@pytest.mark.parametrize("use_gdn,wss", CONFIGS)
def test_one_prepare_twelve_moves_stage_by_stage(worlds, use_gdn, wss):
    """One object over eight slots, ONE prepare, twelve position sets.  Every buffer has guard bands and is filled with random bytes
    before each call — the slots' own workspace blocks too, so what an earlier call left there changes nothing.  Stage by stage:
    the band (the selected streams' symbols, zero elsewhere), the window latent, the pixels; status and flags."""
    wd = worlds(use_gdn, wss)
    rc = wd.rc
    mv = rc.moving_roi(SLOTS)
    coder_ws = int(mv.layout[0].meta_offset)
    assert coder_ws + 64 * len(SLOTS) == mv.ws.numel() and coder_ws == rc.y_coder.ws.numel()
    assert tuple(mv.layout[6].max_streams) == (1, 0) and mv.layout[4].rh_cap == 3 and mv.layout[4].cw_cap == 3     # 1 x 1; an image whole
    outer = _guarded(mv)
    mv.prepare()
    sets, found = _position_sets(wd, mv, seed=wss)
    # the properties of the chosen positions, before any byte is compared
    placed = [[_place(wd, mv, k, x, y) for k, (x, y) in enumerate(xy)] for xy in sets]
    for k, s in enumerate(mv.layout):
        mine = [row[k] for row in placed]
        for t in (0, 1):
            assert max(p.end_stream[t] - p.first_stream[t] for p in mine) == s.max_streams[t], f"slot {k}: set {t}'s capacity is never selected"
        assert max(p.band_rows for p in mine) == s.band_rows_cap
        assert any(p.px.r0 == 0 for p in mine) and any(p.px.r0 == found[k]["last_r0"] == wd.lat[SLOTS[k][0]][1] - s.rh_cap for p in mine)
        assert any((p.px.x0, p.px.y0) == (wd.sizes[SLOTS[k][0]][0] - SLOTS[k][1], wd.sizes[SLOTS[k][0]][1] - SLOTS[k][2]) for p in mine)   # the corner
        if found[k]["surplus"]:
            assert any(-(-(p.end_stream[t] - p.first_stream[t]) // WPB) < s.items[t] for p in mine for t in (0, 1))
        if found[k]["odd"]:
            assert any(p.px.r0 & 1 for p in mine) and any(not p.px.r0 & 1 for p in mine)
    if wss == 1024:
        assert sum(f["surplus"] for f in found) >= 3, "slots whose capacity leaves a whole work item idle somewhere"
    assert sum(f["odd"] for f in found) >= 4
    gen = torch.Generator(device="cuda")
    gen.manual_seed(wss + use_gdn)
    for j, xy in enumerate(sets):
        _randomise(mv, gen, coder_ws)
        out = mv.decode(xy)
        torch.cuda.synchronize()
        st = mv.status.cpu().numpy().astype(np.int64)
        assert not st[:, 0].any(), (j, st)
        assert st[:, 1].tolist() == [p.symbols for p in placed[j]], j
        assert not mv.flags.cpu().numpy().any(), j
        band, lat = mv.band.cpu().numpy(), mv.latent.cpu().numpy()
        at = 0
        for k, ((i, _, _), s, p) in enumerate(zip(SLOTS, mv.layout, placed[j])):
            # 1: the band, over its whole capacity, and the padding in front of it
            a, want = int(s.band_offset), _expected_band(wd, mv, k, p)
            assert not band[at:a].any(), f"set {j}: bytes in front of band {k}"
            assert np.array_equal(band[a:a + want.size], want), f"set {j} slot {k}: band"
            at = a + want.size
            # 2: the window latent
            rh, cw = int(s.rh_cap), int(s.cw_cap)
            got = lat[int(s.latent_offset):int(s.latent_offset) + rh * cw * LAT_C].reshape(rh, cw, LAT_C)
            assert np.array_equal(got, wd.latents[i][p.px.r0:p.px.r0 + rh, p.px.c0:p.px.c0 + cw]), f"set {j} slot {k}: window latent"
        assert not band[at:].any()
        # 3: the ROI pixels
        _check_pixels(mv, wd, xy, out)
    mv.check()
    _guards_untouched(outer)


@pytest.mark.parametrize("use_gdn,wss", [pytest.param(True, 1024, id="gdn-1024"), pytest.param(False, 16384, id="relu-16384")])
def test_clamped_positions(worlds, use_gdn, wss):
    wd = worlds(use_gdn, wss)
    mv = wd.rc.moving_roi(SLOTS)
    mv.prepare()
    rng = np.random.default_rng(5)
    inside = [(int(rng.integers(0, wd.sizes[i][0] - w + 1)), int(rng.integers(0, wd.sizes[i][1] - h + 1))) for i, w, h in SLOTS]
    outside = [(-1, 5), (INT32_MAX, 3), (7, -9), (INT32_MIN, INT32_MIN), (33, 0), (3, INT32_MAX), (1, 0), (INT32_MAX, INT32_MAX)]
    for pick in (range(0, 8, 2), range(1, 8, 2), range(8)):
        xy = [outside[k] if k in pick else inside[k] for k in range(8)]
        want = [int(c != (x, y)) for c, (x, y) in zip(_clamp(wd, SLOTS, xy), xy)]
        assert sum(want) >= 4
        out = mv.decode(torch.tensor(xy, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        assert mv.flags.cpu().tolist() == want == [p["flags"] for p in mv.place(xy)]
        assert not mv.status[:, 0].any()
        _check_pixels(mv, wd, xy, out)                                       # the clamped rectangles, and the other slots unaffected
        first = out.clone()
        again = mv.decode(_clamp(wd, SLOTS, xy))
        torch.cuda.synchronize()
        assert torch.equal(again, first) and not mv.flags.any()              # the bytes of the clamped rectangle itself


@pytest.mark.parametrize("use_gdn,wss", CONFIGS)
def test_equal_to_ragged_hyperprior_roi_with_one_slot_per_image(worlds, use_gdn, wss):
    wd = worlds(use_gdn, wss)
    rc = wd.rc
    slots = [(0, 20, 20), (1, 33, 15), (2, 16, 16), (3, 100, 15), (4, 16, 16)]
    mv = rc.moving_roi(slots)
    mv.prepare()
    for xy in ([(40, 50), (33, 41), (0, 0), (0, 20), (0, 0)], [(572, 572), (127, 625), (32, 32), (0, 21), (0, 0)], [(0, 0)] * 5):
        got = mv.decode(xy).clone()                                          # (the other object's decode runs the front half again)
        roi = rc.roi([(x, y, w, h) for (_, w, h), (x, y) in zip(slots, xy)])
        want = roi.decode()
        torch.cuda.synchronize()
        assert torch.equal(got.reshape(-1), want)
        assert not mv.status[:, 0].any() and not roi.status[:, 0].any()
    uni = rc.moving_roi([(0, 33, 15), (3, 33, 15), (0, 33, 15), (1, 33, 15)])
    uni.prepare()
    xy = [(5, 100), (60, 20), (79, 0), (0, 116)]
    out = uni.decode(xy)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (4, 15, 33, 3) and out.data_ptr() == uni.roi.data_ptr()
    for got, (i, w, h), (x, y) in zip(out.cpu().numpy(), uni.slots, xy):
        assert np.array_equal(got, wd.recons[i][y:y + h, x:x + w])


# ---- verdicts -----------------------------------------------------------------------------------------------------------------------
def _streams(wd, i):
    """(offset of the length table, total streams, anchor streams, the length table) of y container i."""
    im = wd.rc.y_coder.images[i]
    na, ns = int(im.anchor_streams), int(im.anchor_streams) + int(im.nonanchor_streams)
    c = np.frombuffer(wd.containers[i][1], np.uint8)
    return HEADER + TABLES, ns, na, c[HEADER + TABLES:HEADER + TABLES + 4 * ns].view(np.uint32)


def _with_y(wd, i, patch):
    """The y containers with image i's replaced by patch(bytearray)."""
    ys = [y for _, y in wd.containers]
    c = bytearray(ys[i])
    patch(c)
    ys[i] = bytes(c)
    return ys


@pytest.mark.parametrize("which", ["anchor", "non-anchor"])
def test_a_damaged_stream_is_reported_by_the_slot_that_moves_onto_it_and_forgotten_when_it_leaves(worlds, which):
    from simple_image_compression_network_amd import _lib
    wd = worlds(False, 1024)
    slots = [(0, 20, 20), (1, 33, 15), (0, 20, 20), (3, 33, 15)]
    mv = wd.rc.moving_roi(slots)
    table, ns, na, lens = _streams(wd, 0)
    st_bad = 0 if which == "anchor" else na                                  # the first stream of its set: latent rows 0 and 1
    middle = table + 4 * ns + int(lens[:st_bad].sum()) + int(lens[st_bad]) // 2

    def flip(c):
        c[middle] ^= 0x5A
    away = [(40, 572), (33, 41), (300, 572), (60, 10)]                       # both slots of image 0 on its last rows
    onto = [(40, 0), (33, 41), (300, 572), (60, 10)]                         # slot 0 moved to the top
    t = 0 if which == "anchor" else 1
    for k in (0, 2):
        assert _place(wd, mv, k, *away[k]).first_stream[t] > 0
    p = _place(wd, mv, 0, *onto[0])
    assert p.first_stream[t] == 0 < p.end_stream[t]
    mv.prepare(y_containers=_with_y(wd, 0, flip))                            # ONE prepare for the four moves

    def run(xy):
        out = mv.decode(xy)
        torch.cuda.synchronize()
        return mv.status[:, 0].cpu().tolist(), out

    st, out = run(away)                                                      # outside every window: not read, not reported
    assert st == [0, 0, 0, 0]
    _check_pixels(mv, wd, away, out)
    mv.check()
    st, out = run(onto)                                                      # moved onto it: that slot alone
    assert st == [32, 0, 0, 0]
    _check_pixels(mv, wd, onto, out, which=(1, 2, 3))                        # the other slot of the same image stays clean and exact
    with pytest.raises(_lib.SicnError) as e:
        mv.check()
    assert (e.value.slot, e.value.image) == (0, 0)
    st, out = run(away)                                                      # moved off again: the slot's error word was reset
    assert st == [0, 0, 0, 0]
    _check_pixels(mv, wd, away, out)
    mv.prepare()                                                             # and the undamaged containers decode there
    st, out = run(onto)
    assert st == [0, 0, 0, 0]
    _check_pixels(mv, wd, onto, out)


def _patches(ns):
    table = HEADER + TABLES
    yield "magic", 0, 0x4C434954, True
    yield "version-mode", 4, 1 | (3 << 16), True
    yield "image-width (no error)", 8, 7, True
    for k, name in ((16, "lat_w"), (20, "lat_h"), (24, "lat_c"), (28, "n_symbols"), (32, "n_streams"), (36, "stream_symbols")):
        yield name, k, "+1", True
    yield "payload-field huge", 40, 0x7FFFFFF0, True
    yield "checksum (bit 7 in the full decoder, nothing here)", 44, "+1", True
    yield "class table", HEADER + 7 * 256 + 6, "+1", False
    yield "length entry above the cap", table + 4 * 3, 2 * 1024 + 256 + 2, True
    yield "length entry + 2", table + 4 * 2, "+2", False
    yield "length entry - 2", table + 4 * (ns - 1), "-2", False


def test_patched_fixed_parts_give_the_full_decoders_status_without_bit_7(worlds):
    """Image 1 whole in slot 1 — every stream selected — and two small rectangles of it; its y container's fixed part patched field
    by field.  The whole-image slot reports what the full decoder reports, bit 7 masked.  So do the small slots wherever the
    verdict does not hang on WHICH streams were read (`everywhere`); where it does — a class whose table is refused, a length entry
    that moves the streams behind it — they agree on every bit but 5, which by the header's rule speaks of the selected streams
    alone.  The slots of other images stay clean and exact."""
    wd = worlds(False, 1024)
    rc = wd.rc
    slots = [(0, 20, 20), (1, 160, 640), (3, 33, 15), (1, 1, 1), (1, 33, 15)]
    xy = [(40, 50), (0, 0), (60, 10), (50, 630), (100, 300)]
    mv = rc.moving_roi(slots)
    _, ns, _, _ = _streams(wd, 1)
    seen = set()
    for name, off, value, everywhere in _patches(ns):
        def patch(c):
            old = int.from_bytes(c[off:off + 4], "little")
            new = (old + int(value)) & 0xFFFFFFFF if isinstance(value, str) else value
            c[off:off + 4] = new.to_bytes(4, "little")
        damaged = _with_y(wd, 1, patch)
        rc.decode(y_containers=damaged)                                      # the full decoder of the same bytes
        torch.cuda.synchronize()
        want = int(rc.y_coder.dec_status[1, 0].item())
        mv.prepare(y_containers=damaged)
        out = mv.decode(xy)
        torch.cuda.synchronize()
        got = mv.status.cpu().numpy().astype(np.int64)
        assert got[1, 0] == want & ~128, f"{name}: the whole-image slot {got[1, 0]}, full decoder {want}"
        for k in (3, 4):
            if everywhere:
                assert got[k, 0] == want & ~128, f"{name}: slot {k} {got[k, 0]}, full decoder {want}"
            else:
                assert got[k, 0] & ~32 == want & ~(128 | 32) and (want & 32 or not got[k, 0] & 32), f"{name}: slot {k} {got[k, 0]}, full decoder {want}"
        assert got[0, 0] == got[2, 0] == 0, name
        _check_pixels(mv, wd, xy, out, which=(0, 2))
        seen.add(want)
    assert {0, 128} <= seen and any(s & 4 for s in seen) and any(s & 8 for s in seen) and any(s & 16 for s in seen)
    assert any(s & 32 for s in seen) and any(s & 64 for s in seen)           # every bit of the fixed part was provoked


def test_valid_shorter_than_the_fixed_part(worlds):
    wd = worlds(False, 1024)
    rc = wd.rc
    slots = [(0, 20, 20), (1, 160, 640), (3, 33, 15), (1, 1, 1)]
    xy = [(40, 50), (0, 0), (60, 10), (50, 630)]
    mv = rc.moving_roi(slots)
    _, ns, _, _ = _streams(wd, 1)
    short = _with_y(wd, 1, lambda c: c.__delitem__(slice(HEADER + TABLES + 4 * ns - 1, None)))
    assert len(short[1]) == HEADER + TABLES + 4 * ns - 1
    rc.decode(y_containers=short)
    torch.cuda.synchronize()
    want = rc.y_coder.dec_status[:, 0].cpu().tolist()
    mv.prepare(y_containers=short)
    out = mv.decode(xy)
    torch.cuda.synchronize()
    st = mv.status[:, 0].cpu().tolist()
    assert want[1] & 0x104 == 0x104 and st == [0, want[1] & ~128, 0, want[1] & ~128]
    band = mv.band.cpu().numpy()
    for k in (1, 3):                                                         # the refused image's slots decoded nothing
        a = int(mv.layout[k].band_offset)
        assert not band[a:a + int(mv.layout[k].band_rows_cap) * 10 * LAT_C].any()
    _check_pixels(mv, wd, xy, out, which=(0, 2))


# ---- no non-anchor capacity, archive, graph, memory -----------------------------------------------------------------------------------
def test_a_batch_of_1x1_latents_skips_the_non_anchor_launch(worlds):
    wd = worlds(False, 1024, sizes=[(16, 16)] * 3)
    mv = wd.rc.moving_roi([(1, 16, 16), (0, 7, 5), (2, 16, 16), (1, 1, 1)])
    assert mv.items == (4, 0) and all(tuple(s.max_streams) == (1, 0) for s in mv.layout)
    mv.prepare()
    for xy in ([(0, 0)] * 4, [(0, 0), (9, 11), (0, 0), (15, 15)], [(5, 5), (3, 0), (-4, 2), (7, 8)]):
        out = mv.decode(xy)
        torch.cuda.synchronize()
        assert mv.status.cpu().tolist() == [[0, LAT_C]] * 4
        _check_pixels(mv, wd, xy, out)


def test_an_archive_unpacked_once_serves_many_moves(worlds):
    from simple_image_compression_network_amd import hyperprior
    wd = worlds(True, 1024)
    blob = wd.rc.archive()
    sel = [0, 1, 3]
    rc = hyperprior.RaggedHyperpriorCodec.from_archive(blob, seed=SEED, images=sel)
    assert rc.sizes == [SIZES[i] for i in sel] and list(rc.y_coder.stream_symbols) == [1024] * 3 and rc.use_gdn
    slots = [(2, 64, 16), (0, 20, 20), (1, 33, 15), (0, 20, 20)]
    mv = rc.moving_roi(slots)
    mv.prepare(archive=blob, images=sel)                                     # once
    for xy in ([(0, 0)] * 4, [(36, 20), (572, 572), (127, 625), (0, 572)], [(10, 7), (41, 77), (13, 60), (55, 3)], [(31, 15), (16, 16), (32, 32), (17, 31)]):
        out = mv.decode(xy)
        mv.check()
        for v, (i, w, h), (x, y) in zip(mv.views(out), slots, xy):
            assert np.array_equal(v.cpu().numpy(), wd.recons[sel[i]][y:y + h, x:x + w]), (xy, i)


def test_a_captured_chain_replays_with_positions_drawn_on_the_device(worlds):
    wd = worlds(True, 1024)
    slots = [(1, 33, 15), (0, 20, 20), (3, 33, 15), (0, 16, 16), (4, 16, 16)]
    mv = wd.rc.moving_roi(slots)                                             # every object is made and prepared before the capture
    mv.prepare()
    last = torch.tensor([[wd.sizes[i][0] - w, wd.sizes[i][1] - h] for i, w, h in slots], dtype=torch.int32, device="cuda")
    xy = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    mv.decode(xy)                                                            # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = mv.decode(xy)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for _ in range(2):
        drawn = (torch.rand((5, 2), device="cuda", generator=gen) * (last + 1).float()).to(torch.int32).clamp_(max=last)   # on the device
        xy.copy_(drawn)
        out.fill_(PATTERN)
        mv.status.fill_(-1)
        mv.flags.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        host = xy.cpu().tolist()
        assert not mv.status[:, 0].any() and not mv.flags.any()
        _check_pixels(mv, wd, host, out)
    xy.copy_(torch.tensor([[10, 700], [-3, 60], [200, 33], [50, 50], [0, 0]], dtype=torch.int32, device="cuda"))
    graph.replay()
    torch.cuda.synchronize()
    host = xy.cpu().tolist()
    assert mv.flags.cpu().tolist() == [int(c != tuple(p)) for c, p in zip(_clamp(wd, slots, host), host)] == [1, 1, 1, 0, 0]
    _check_pixels(mv, wd, host, out)


def test_decode_allocates_nothing(worlds):
    wd = worlds(True, 1024)
    mv = wd.rc.moving_roi(SLOTS)
    mv.prepare()
    xy_dev = torch.zeros((len(SLOTS), 2), dtype=torch.int32, device="cuda")
    host = [(1, 2)] * len(SLOTS)
    mv.decode(xy_dev)                                                        # the first call
    torch.cuda.synchronize()
    for xy in (xy_dev, host, xy_dev, host):
        before = torch.cuda.memory_allocated()
        out = mv.decode(xy)
        after = torch.cuda.memory_allocated()
        torch.cuda.synchronize()
        assert after == before == torch.cuda.memory_allocated()
        assert out.data_ptr() == mv.roi.data_ptr()
    _check_pixels(mv, wd, host, out)


def test_decode_before_prepare_raises_and_bad_arguments_are_refused(worlds):
    wd = worlds(False, 1024)
    mv = wd.rc.moving_roi([(0, 20, 20), (1, 33, 15)])
    with pytest.raises(RuntimeError, match="prepare"):
        mv.decode([(0, 0), (0, 0)])
    mv.prepare()
    for bad in ([(0, 0)] * 3, torch.zeros((2, 2), dtype=torch.int64, device="cuda"), torch.zeros((1, 4), dtype=torch.int32, device="cuda")):
        with pytest.raises((ValueError, TypeError)):
            mv.decode(bad)
    for bad in ([], [(5, 20, 20)], [(0, 593, 20)], [(0, 20, 593)], [(0, 0, 20)], [(0, 20)]):
        with pytest.raises(ValueError):
            wd.rc.moving_roi(bad)
    with pytest.raises(ValueError):
        mv.prepare(images=[0, 1])                                            # images= selects from an archive


def test_argument_checks_come_before_any_launch(worlds):
    from simple_image_compression_network_amd import _lib
    L = _lib.lib()
    wd = worlds(False, 1024)
    rc = wd.rc
    mv = rc.moving_roi(SLOTS)
    outer = _guarded(mv)
    mv.prepare()
    torch.cuda.synchronize()
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    xy = torch.zeros((len(SLOTS), 2), dtype=torch.int32, device="cuda")
    need = int(L.sicn_ragged_ctx_roi_move_workspace_bytes(mv._h))
    assert need == mv.ws.numel() == rc.y_coder.ws.numel() + 64 * len(SLOTS)
    ws_before = mv.ws.clone()
    names = ("band", "latent", "status", "flags")
    for name in names:
        getattr(mv, name).view(-1).view(torch.uint8).fill_(PATTERN)
    slots_buf = rc.y_coder.slot_buffer
    args = [mv._h, ptr(xy), ptr(slots_buf), ptr(rc.s), ptr(mv.band), ptr(mv.latent), ptr(mv.status), ptr(mv.flags), ptr(mv.ws)]
    call = L.sicn_ragged_ctx_roi_move_decode_async
    assert call(*args, need - 1, stream) == -28
    assert call(*args[:8], ptr(mv.ws, 8), need, stream) == -22
    assert call(*args[:1], ptr(xy, 2), *args[2:], need, stream) == -22
    assert call(*args[:2], ptr(slots_buf, 1), *args[3:], need, stream) == -22
    assert call(*args[:3], ptr(rc.s, 2), *args[4:], need, stream) == -22
    assert call(*args[:4], ptr(mv.band, 2), *args[5:], need, stream) == -22
    for k in range(1, 8):
        assert call(*args[:k], None, *args[k + 1:], need, stream) == -22, k
    prep = L.sicn_ragged_ctx_roi_move_prepare_async
    assert prep(mv._h, ptr(slots_buf), None, ptr(mv.ws), need - 1, stream) == -28
    assert prep(mv._h, ptr(slots_buf, 1), None, ptr(mv.ws), need, stream) == -22
    assert prep(mv._h, ptr(slots_buf), None, ptr(mv.ws, 8), need, stream) == -22
    assert prep(mv._h, None, None, ptr(mv.ws), need, stream) == -22
    torch.cuda.synchronize()
    for name in names:                                                       # nothing was enqueued
        assert (getattr(mv, name).view(-1).view(torch.uint8).cpu().numpy() == PATTERN).all(), name
    assert torch.equal(mv.ws, ws_before)
    assert call(*args, need, stream) == 0
    torch.cuda.synchronize()
    assert not mv.status[:, 0].any()
    _guards_untouched(outer)


def test_create_refuses_a_bad_second_slot_and_leaves_no_handle():
    """sicn_ragged_ctx_roi_move_create over a live coder of two images (16 x 16 and 48 x 32: latents 1 x 1 and 3 x 2, 4 channels):
    a SECOND slot its image cannot hold is refused after the first slot was laid out — SICN_EINVAL and a null handle — and the same
    coder then makes an object of sound slots."""
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import _lib
    L = _lib.lib()
    u32 = ctypes.c_uint32 * 2
    coder, mv = ctypes.c_void_p(), ctypes.c_void_p(1)
    assert L.sicn_ragged_ctx_coder_create(u32(1, 3), u32(1, 2), 4, u32(16, 48), u32(16, 32), 2, ctypes.byref(coder)) == 0
    try:
        for bad in [(1, 49, 20), (1, 20, 0), (2, 16, 16)]:                           # wider than its image; empty; no such image
            mv.value = 1
            slots = (_lib.RaggedRoiSlot * 2)(_lib.RaggedRoiSlot(0, 16, 16), _lib.RaggedRoiSlot(*bad))
            assert L.sicn_ragged_ctx_roi_move_create(coder, slots, 2, ctypes.byref(mv)) == -22
            assert not mv.value
        slots = (_lib.RaggedRoiSlot * 2)(_lib.RaggedRoiSlot(0, 16, 16), _lib.RaggedRoiSlot(1, 20, 20))
        assert L.sicn_ragged_ctx_roi_move_create(coder, slots, 2, ctypes.byref(mv)) == 0 and mv.value
        assert L.sicn_ragged_ctx_roi_move_workspace_bytes(mv) > 0
        L.sicn_ragged_ctx_roi_move_free(mv)
    finally:
        L.sicn_ragged_ctx_coder_free(coder)
