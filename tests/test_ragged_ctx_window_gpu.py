"""GPU checks of the hyperprior window decoder (include/sicn_ragged_ctx_window.h, codec.RaggedContextWindowDecoder; run with -m gpu on
an MI355X): a window of latent rows of each image of a ragged batch from its rANS-WC streams.  Everything is byte equality: the
containers are the C oracle's, the expected band is the original latent with every symbol outside the selected streams zeroed, by
the numpy statement of the set order in tests/codec_edge_cases.py."""
import ctypes
import functools

import numpy as np
import pytest

import codec_edge_cases as ce
from oracle import c_oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LAT_C = 192
# 37 x 37: 9 + 9 streams, odd W and H.  86 x 86: 44 + 44 streams — selections start off a multiple of the decoder's group of eight
# and span several groups.  3 x 3 and 5 x 1: single-stream images; 5 x 1 has non-anchors but no horizontal neighbours.
SHAPES = [(37, 37), (40, 48), (3, 3), (86, 86), (5, 1)]
CONTENT = ["uniform-uniform", "peaked", "checkerboard", "peaked", "tie-up"]
GUARD, PATTERN = 4096, 0xA5
# per case, (r0, rh) per image
WINDOWS = {
    "top": [(0, 3), (0, 5), (0, 1), (0, 4), (0, 2)],
    "bottom": [(34, 3), (35, 5), (2, 1), (80, 6), (3, 2)],
    "one-row-odd": [(17, 1), (21, 1), (1, 1), (43, 1), (3, 1)],
    "one-row-even": [(18, 1), (20, 1), (2, 1), (44, 1), (2, 1)],
    "whole": [(0, h) for h, _ in SHAPES],
    "middle": [(11, 9), (14, 7), (1, 1), (39, 8), (1, 3)],
}
HEADER, TABLES = ce.HEADER, ce.CTX_TABLES


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import codec as _codec
    return _codec


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _pack(arrays):
    return _dev(np.concatenate([a.reshape(-1) for a in arrays]))


@functools.lru_cache(maxsize=None)
def _batch():
    """([y], [s], [oracle container], [(set, stream) of every symbol]); computed once, never modified."""
    rng = np.random.default_rng(913)
    ys, ss, where = [], [], []
    for (h, w), name in zip(SHAPES, CONTENT):
        shape = (h, w, LAT_C)
        s = rng.integers(0, 128, shape, dtype=np.uint8)
        if name == "peaked":
            y = np.minimum((rng.exponential(1.0, shape) * (s / 8 + 0.5)).astype(np.int64), 127).astype(np.uint8)
        else:
            y = np.array(ce.CTX_CONTENTS[name](shape, rng)[0])
        index = np.arange(y.size, dtype=np.int64).reshape(shape)
        order = ce.ctx_set_order(index)
        pos = np.empty(y.size, np.int64)
        pos[order] = np.arange(y.size)
        pos = pos.reshape(shape)
        anchor, _ = ce.ctx_masks(h, w)
        na = ce.ctx_geometry(h, w, LAT_C)[0][0]
        pset = np.broadcast_to(~anchor[:, :, None], shape)
        stream = np.where(pset, pos - na, pos) // ce.WSS
        for a in (y, s, stream):
            a.setflags(write=False)
        ys.append(y); ss.append(s); where.append((pset, stream))
    blobs = [c_oracle.ctx_encode(y, s, (16 * w, 16 * h)) for y, s, (h, w) in zip(ys, ss, SHAPES)]
    return ys, ss, blobs, where


@pytest.fixture(scope="module")
def setup(codec):
    ys, ss, blobs, _ = _batch()
    coder = codec.RaggedContextCoder.for_containers(blobs)
    assert coder.shapes == SHAPES
    return coder, _pack(ss), _pack(ys)


def _expected(win, i):
    """(band, wanted rows) of image i: the original latent rows of the band, zero where a symbol's stream is not selected."""
    ys, _, _, where = _batch()
    im = win.images[i]
    pset, stream = where[i]
    first, end = np.array(list(im.first_stream)), np.array(list(im.end_stream))
    held = (stream >= first[pset.astype(np.int64)]) & (stream < end[pset.astype(np.int64)])
    b0, rows = int(im.band_row0), int(im.band_rows)
    r0, rh = win.rows[i]
    assert held[r0:r0 + rh].all() and int(held.sum()) == int(im.symbols)
    return np.where(held, ys[i], 0).astype(np.uint8)[b0:b0 + rows], ys[i][r0:r0 + rh]


def _check_band(win, band, skip=()):
    host = band.cpu().numpy()
    views = win.views(band)
    for i, im in enumerate(win.images[:len(SHAPES)]):
        if i in skip:
            continue
        want, rows = _expected(win, i)
        got = host[int(im.band_offset):int(im.band_offset) + int(im.band_bytes)].reshape(want.shape)
        assert np.array_equal(got, want), f"image {i} {SHAPES[i]}: band"
        assert np.array_equal(views[i].cpu().numpy(), rows), f"image {i}: views()"
    return host


@pytest.mark.parametrize("case", list(WINDOWS))
def test_window_equals_the_latent_rows(setup, case):
    coder, sd, _ = setup
    win = coder.window(WINDOWS[case])
    assert win.band_bytes == sum(-(-int(im.band_bytes) // 16) * 16 for im in win.images[:len(SHAPES)])
    outs = []
    for fill in (0xEE, 0x00):                                        # the result is independent of the band's previous fill
        band = torch.full((win.band_bytes,), fill, dtype=torch.uint8, device="cuda")
        win.status.fill_(-1)
        win.decode(band, sd)
        win.check()
        assert win.status.cpu().tolist() == [[0, int(im.symbols)] for im in win.images[:len(SHAPES)]]
        outs.append(_check_band(win, band))
    assert np.array_equal(outs[0], outs[1])
    if case == "whole":
        assert win.selected_streams == sum(int(im.anchor_streams) + int(im.nonanchor_streams) for im in coder.images[:len(SHAPES)])
        assert win.band_bytes == sum(-(-h * w * LAT_C // 16) * 16 for h, w in SHAPES)
    else:
        assert win.selected_streams < sum(int(im.anchor_streams) + int(im.nonanchor_streams) for im in coder.images[:len(SHAPES)])


def test_window_stays_inside_its_buffers(setup):
    """Band tensor, workspace and status between guard bands of 4096 bytes of 0xA5: every guard byte intact."""
    from simple_image_compression_network_amd import _lib
    coder, sd, _ = setup
    win = coder.window(WINDOWS["middle"])
    L = _lib.lib()
    sizes = {"band": win.band_bytes, "ws": int(L.sicn_ragged_ctx_window_workspace_bytes(win._h)), "status": 8 * len(SHAPES)}
    assert sizes["ws"] == int(L.sicn_ragged_ctx_coder_workspace_bytes(coder._h))
    buf = {k: torch.full((GUARD + v + GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    ptr = {k: ctypes.c_void_p(t.data_ptr() + GUARD) for k, t in buf.items()}
    rc = L.sicn_ragged_ctx_window_decode_async(win._h, ctypes.c_void_p(coder.slot_buffer.data_ptr()), ctypes.c_void_p(coder.enc_status.data_ptr()),
                                               ctypes.c_void_p(sd.data_ptr()), ptr["band"], ptr["status"], ptr["ws"], sizes["ws"],
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for name, t in buf.items():
        hst = t.cpu().numpy()
        assert (hst[:GUARD] == PATTERN).all() and (hst[GUARD + sizes[name]:] == PATTERN).all(), f"guard band of `{name}` was written"
    _check_band(win, buf["band"][GUARD:GUARD + sizes["band"]])
    status = buf["status"][GUARD:GUARD + sizes["status"]].cpu().numpy().view("<i4").reshape(-1, 2).tolist()
    assert status == [[0, int(im.symbols)] for im in win.images[:len(SHAPES)]]


def _stream_offsets(blob):
    """Byte offsets of every stream's payload inside a container (anchors, then non-anchors)."""
    _, _, lens = ce.ctx_container_fields(blob)
    base = ce.CTX_LENS + 4 * lens.size
    return base + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), lens


def _decode_both(coder, win, sd, slots, valid):
    """The window decoder and the full decoder on the same (damaged) slots: (window status, full status, band, full latents)."""
    band = torch.full((win.band_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    back = torch.full((coder.latent_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    win.status.fill_(-1)
    coder.dec_status.fill_(-1)
    win.decode(band, sd, slots=slots, valid=valid)
    coder.decode(back, sd, slots=slots, valid=valid)
    torch.cuda.synchronize()
    return win.status.cpu().tolist(), coder.dec_status.cpu().tolist(), band, back


BAD = 3            # the 86 x 86 image: 44 + 44 streams


@pytest.mark.parametrize("which", ["anchor", "non-anchor"])
def test_a_flipped_payload_byte(setup, which):
    coder, sd, _ = setup
    _, _, blobs, _ = _batch()
    win = coder.window(WINDOWS["middle"])
    im, cim = win.images[BAD], coder.images[BAD]
    s = 0 if which == "anchor" else 1
    na = int(cim.anchor_streams)
    assert 0 < im.first_stream[s] < im.end_stream[s] < (na, int(cim.nonanchor_streams))[s]      # streams on both sides of the window
    offs, lens = _stream_offsets(blobs[BAD])
    # in an unselected stream before and one behind the window: status 0 and equal bytes
    for st in (0, (na, int(cim.nonanchor_streams))[s] - 1):
        g = st + s * na
        slots = coder.slot_buffer.clone()
        slots[int(cim.slot_offset) + int(offs[g]) + int(lens[g]) // 2] ^= 0x40
        wst, fst, band, _ = _decode_both(coder, win, sd, slots, coder.enc_status)
        assert wst == [[0, int(i.symbols)] for i in win.images[:len(SHAPES)]], (which, st)
        assert fst[BAD][0] == 32 and all(fst[i][0] == 0 for i in range(len(SHAPES)) if i != BAD)   # the full decoder reads it
        _check_band(win, band)
    # in a selected stream: bit 5 for that image alone, neighbours exact
    g = int(im.first_stream[s]) + 1 + s * na
    slots = coder.slot_buffer.clone()
    slots[int(cim.slot_offset) + int(offs[g]) + int(lens[g]) // 2] ^= 0x40
    wst, fst, band, _ = _decode_both(coder, win, sd, slots, coder.enc_status)
    assert wst == [[32 if i == BAD else 0, int(x.symbols)] for i, x in enumerate(win.images[:len(SHAPES)])]
    assert fst[BAD][0] == 32
    _check_band(win, band, skip=(BAD,))


def _patched(coder, name):
    """(slots, valid, the bit the damage must raise) with image BAD's container damaged as `name` says."""
    cim = coder.images[BAD]
    base = int(cim.slot_offset)
    slots, valid = coder.slot_buffer.clone(), coder.enc_status.clone()
    ns = int(cim.anchor_streams) + int(cim.nonanchor_streams)
    if name == "header-dword":                       # lat_w
        slots[base + 16] ^= 0x01
        return slots, valid, 4
    if name == "class-table":                        # one frequency of class 0 more: the table no longer sums to 4096
        host = slots[base + HEADER:base + HEADER + 256].cpu().numpy().view("<u2").copy()
        k = int(np.nonzero(host)[0][0])
        host[k] += 1
        slots[base + HEADER:base + HEADER + 256] = _dev(host.view(np.uint8))
        return slots, valid, 8
    if name == "payload-field":                      # more payload than the valid bytes hold
        slots[base + 40:base + 44] = _dev(np.array([0x7FFFFFFF], "<u4").view(np.uint8))
        return slots, valid, 16
    if name == "length-entry-above-cap":             # of the LAST non-anchor stream, outside the window
        at = base + HEADER + TABLES + 4 * (ns - 1)
        slots[at:at + 4] = _dev(np.array([2 * ce.WSS + 256 + 2], "<u4").view(np.uint8))
        return slots, valid, 32
    assert name == "valid-short-of-the-fixed-part"
    valid[BAD, 1] = HEADER + TABLES + 4 * ns - 1
    return slots, valid, 0x104


@pytest.mark.parametrize("name", ["header-dword", "class-table", "payload-field", "length-entry-above-cap", "valid-short-of-the-fixed-part"])
def test_a_damaged_fixed_part_is_reported_as_the_full_decoder_reports_it(setup, name):
    coder, sd, yd = setup
    win = coder.window(WINDOWS["middle"])
    slots, valid, bits = _patched(coder, name)
    wst, fst, band, back = _decode_both(coder, win, sd, slots, valid)
    assert [e for e, _ in wst] == [e & ~128 for e, _ in fst], (wst, fst)
    assert wst[BAD][0] & bits == bits and not wst[BAD][0] & 128
    assert all(wst[i] == [0, int(win.images[i].symbols)] for i in range(len(SHAPES)) if i != BAD)
    _check_band(win, band, skip=(BAD,))
    with pytest.raises(RuntimeError) as e:
        win.check()
    assert e.value.image == BAD
    # the rejected image's band does not depend on what the buffer held
    other = torch.zeros_like(band)
    win.decode(other, sd, slots=slots, valid=valid)
    torch.cuda.synchronize()
    assert torch.equal(other, band)


def test_window_captured_in_a_graph_and_replayed(setup):
    coder, sd, _ = setup
    win = coder.window(WINDOWS["middle"])
    band = torch.full((win.band_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    win.decode(band, sd)                                           # warm-up: module load
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            win.decode(band, sd)
    for fill in (0x5A, 0xFF):
        band.fill_(fill)
        win.status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert win.status.cpu().tolist() == [[0, int(im.symbols)] for im in win.images[:len(SHAPES)]]
        _check_band(win, band)


def test_window_and_full_decoder_alternate_on_one_coder(setup):
    coder, sd, yd = setup
    wins = [coder.window(WINDOWS["middle"]), coder.window(WINDOWS["one-row-odd"])]
    for win in wins + wins[::-1]:
        band = torch.full((win.band_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
        win.decode(band, sd)
        back = torch.full_like(yd, 0xEE)
        coder.decode(back, sd)
        win.check()
        coder.check()
        _check_band(win, band)
        assert torch.equal(back, yd)
        assert coder.dec_status.cpu().tolist() == [[0, h * w * LAT_C] for h, w in SHAPES]


def test_window_create_refuses_a_bad_second_image_and_leaves_no_handle(codec):
    """sicn_ragged_ctx_window_create over a live coder of two images (latents 1 x 1 and 3 x 2, 4 channels): a row range the SECOND
    image cannot hold is refused after the first image's entries were made — SICN_EINVAL and a null handle — and the same coder then
    makes a window of sound rows."""
    from simple_image_compression_network_amd import _lib
    L = _lib.lib()
    u32 = ctypes.c_uint32 * 2
    coder, win = ctypes.c_void_p(), ctypes.c_void_p(1)
    assert L.sicn_ragged_ctx_coder_create(u32(1, 3), u32(1, 2), 4, None, None, 2, ctypes.byref(coder)) == 0
    try:
        for r0, rh in [((0, 0), (1, 0)), ((0, 2), (1, 1)), ((0, 1), (1, 2))]:       # no rows; behind the latent; past its end
            win.value = 1
            assert L.sicn_ragged_ctx_window_create(coder, u32(*r0), u32(*rh), ctypes.byref(win)) == -22
            assert not win.value
        assert L.sicn_ragged_ctx_window_create(coder, u32(0, 1), u32(1, 1), ctypes.byref(win)) == 0 and win.value
        assert L.sicn_ragged_ctx_window_workspace_bytes(win) == L.sicn_ragged_ctx_coder_workspace_bytes(coder)
        L.sicn_ragged_ctx_window_free(win)
    finally:
        L.sicn_ragged_ctx_coder_free(coder)
