"""GPU checks of the rANS-WC stream length as an encoder parameter (include/sicn_ctx_stream_length.h): the uniform _sl entry points,
the ragged coder with a length per image, the window decoder and the hyperprior codecs at 1024 .. 16384.  Byte equality throughout
against tests/cpp/ctx_sl_reference.c, which tests/test_ctx_stream_length.py holds to the oracle."""
import ctypes

import numpy as np
import pytest

import ctx_sl_cases as sl
from oracle import c_oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD, PATTERN = 4096, 0xA5
EDGES = [(16, 32, 4), (16, 33, 4), (17, 32, 4), (1, 1, 4), (1, 5, 8), (3, 3, 4)]
BIG = [(37, 37, 192), (40, 48, 192)]
MIXED, MIXED_LENGTHS = [(37, 37, 192), (12, 16, 192), (40, 48, 192)], [1024, 16384, 4096]


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import codec as _codec
    return _codec


@pytest.fixture(scope="module")
def lib(codec):
    from simple_image_compression_network_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _pack(arrays):
    return _dev(np.concatenate([np.asarray(a).reshape(-1) for a in arrays]))


def _wh(shapes):
    return [sl.image_wh((h, w, 0)) for h, w in shapes]


class Guarded:
    """A device buffer of `nbytes` (rounded up to 16) between two guard bands of a pattern nobody writes."""
    def __init__(self, nbytes, fill=0):
        self.n = -(-max(nbytes, 1) // 16) * 16
        self.whole = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        self.t = self.whole[GUARD:GUARD + self.n]
        self.t.fill_(fill)

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.whole[:GUARD] == PATTERN).all()) and bool((self.whole[GUARD + self.n:] == PATTERN).all())


def _uniform_sl(lib, y, s, S, containers=None):
    """One image through sicn_codec_ctx_encode_batch_async_sl (unless `containers`: bytes to decode instead) and
    sicn_codec_ctx_decode_batch_async_sl, every buffer between guard bands: (container, encode status, decoded latent, decode status)."""
    L = lib.lib()
    h, w, c = y.shape
    slot = -(-int(L.sicn_codec_ctx_max_bytes_sl(w, h, c, S)) // 2) * 2
    ws = Guarded(int(L.sicn_codec_ctx_workspace_bytes_sl(w, h, c, 1, S)), 0x5A)
    lat, scale, out, back = Guarded(y.size), Guarded(y.size), Guarded(slot, 0xEE), Guarded(y.size, 0xEE)
    lat.t[:y.size] = _dev(y.reshape(-1))
    scale.t[:y.size] = _dev(s.reshape(-1))
    est, dst = Guarded(8, 0xFF), Guarded(8, 0xFF)
    wh = sl.image_wh(y.shape)
    if containers is None:
        rc = L.sicn_codec_ctx_encode_batch_async_sl(lat.ptr(), scale.ptr(), 1, w, h, c, wh[0], wh[1], out.ptr(), slot, est.ptr(), ws.ptr(),
                                                    ws.n, None, S)
        assert rc == 0
        valid = est.ptr()
    else:
        assert len(containers) <= slot
        out.t[:len(containers)] = _dev(np.frombuffer(containers, np.uint8))
        valid = None
    rc = L.sicn_codec_ctx_decode_batch_async_sl(out.ptr(), slot, valid, scale.ptr(), 1, w, h, c, back.ptr(), dst.ptr(), ws.ptr(), ws.n, None, S)
    assert rc == 0
    torch.cuda.synchronize()
    assert all(g.intact() for g in (ws, lat, scale, out, back, est, dst)), "a write outside a buffer"
    e, d = est.t.view(torch.int32)[:2].cpu().tolist(), dst.t.view(torch.int32)[:2].cpu().tolist()
    size = e[1] if containers is None else len(containers)
    return out.t[:size].cpu().numpy().tobytes(), e, back.t[:y.size].cpu().numpy().reshape(y.shape), d


def _ragged(codec, shapes, c, lengths, variants=None):
    """A RaggedContextCoder over sl.latent(shape, variant): encode + decode.  Returns (coder, ys, ss, scales on the device, decoded)."""
    variants = variants or [0] * len(shapes)
    ys, ss = zip(*[sl.latent((h, w, c), v) for (h, w), v in zip(shapes, variants)])
    coder = codec.RaggedContextCoder(shapes, c, _wh(shapes), stream_symbols=lengths)
    coder.enc_status.fill_(-1)
    coder.dec_status.fill_(-1)
    yd, sd = _pack(ys), _pack(ss)
    coder.encode(yd, sd)
    back = torch.full_like(yd, 0xEE)
    coder.decode(back, sd)
    torch.cuda.synchronize()
    return coder, ys, ss, sd, back


# ---- stream-count edges at S = 1024 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EDGES, ids=lambda s: "x".join(map(str, s)))
def test_stream_count_edges_at_1024(codec, lib, shape):
    y, s = sl.latent(shape)
    want = sl.container(shape, 1024)
    got, est, back, dst = _uniform_sl(lib, y, s, 1024)
    assert est == [0, len(want)] and got == want
    assert dst == [0, y.size] and np.array_equal(back, y)
    h, w, c = shape
    coder, _, _, _, rback = _ragged(codec, [(h, w)], c, 1024)
    assert coder.enc_status.cpu().tolist() == [[0, len(want)]] and coder.containers() == [want]
    assert coder.dec_status.cpu().tolist() == [[0, y.size]] and np.array_equal(rback.cpu().numpy().reshape(shape), y)
    nst = sl.geometry(h, w, c, 1024)[1]
    assert (coder.images[0].anchor_streams, coder.images[0].nonanchor_streams) == nst
    if shape == (16, 32, 4):                                  # one full stream per set: the oracle's own container but for dword 9
        o = bytearray(c_oracle.ctx_encode(y, s, sl.image_wh(shape)))
        o[36:40] = (1024).to_bytes(4, "little")
        assert got == bytes(o)


# ---- all five lengths, uniform and ragged, each reading the other's containers ---------------------------------------------------
@pytest.mark.parametrize("S", sl.LENGTHS)
@pytest.mark.parametrize("shape", BIG, ids=lambda s: "x".join(map(str, s)))
def test_every_length_uniform_and_ragged(codec, lib, shape, S):
    y, s = sl.latent(shape)
    h, w, c = shape
    want = sl.container(shape, S)
    got, est, back, dst = _uniform_sl(lib, y, s, S)
    assert est == [0, len(want)] and got == want, "sicn_codec_ctx_encode_batch_async_sl"
    assert dst == [0, y.size] and np.array_equal(back, y)
    coder, _, _, sd, rback = _ragged(codec, [(h, w)], c, S)
    assert coder.stream_symbols == [S] and coder.containers() == [want], "the ragged coder"
    assert coder.dec_status.cpu().tolist() == [[0, y.size]] and np.array_equal(rback.cpu().numpy().reshape(shape), y)
    # the ragged coder's container through the uniform decoder, in place in a slot of the uniform size
    _, _, back2, dst2 = _uniform_sl(lib, y, s, S, containers=coder.containers()[0])
    assert dst2 == [0, y.size] and np.array_equal(back2, y)
    # the uniform coder's container through the ragged decoder (for_containers reads the length from the header)
    other = codec.RaggedContextCoder.for_containers([got])
    assert other.stream_symbols == [S] and other.shapes == [(h, w)]
    out = torch.full((y.size,), 0xEE, dtype=torch.uint8, device="cuda")
    other.decode(out, sd)
    other.check()
    assert np.array_equal(out.cpu().numpy().reshape(shape), y)
    # the Python class of the uniform coder
    one = codec.ContextCoder(1, h, w, c, *sl.image_wh(shape), stream_symbols=S)
    one.encode(_dev(y[None]), _dev(s[None]))
    torch.cuda.synchronize()
    assert one.sizes() == [len(want)] and one.slots[0, :len(want)].cpu().numpy().tobytes() == want
    if S == 16384:                                            # ... and at 16384 the old entry points' bytes and the oracle's
        L = lib.lib()
        slot = int(L.sicn_codec_ctx_max_bytes(w, h, c))
        assert slot == int(L.sicn_codec_ctx_max_bytes_sl(w, h, c, S))
        ws = Guarded(int(L.sicn_codec_ctx_workspace_bytes(w, h, c, 1)))
        o, st, yd = Guarded(slot, 0xEE), Guarded(8, 0xFF), _dev(y)
        wh = sl.image_wh(shape)
        assert L.sicn_codec_ctx_encode_batch_async(ctypes.c_void_p(yd.data_ptr()), ctypes.c_void_p(sd.data_ptr()), 1, w, h, c, wh[0], wh[1],
                                                   o.ptr(), slot, st.ptr(), ws.ptr(), ws.n, None) == 0
        torch.cuda.synchronize()
        assert st.t.view(torch.int32)[:2].cpu().tolist() == [0, len(want)] and ws.intact() and o.intact()
        assert o.t[:len(want)].cpu().numpy().tobytes() == want == c_oracle.ctx_encode(y, s, wh)
        plain = codec.RaggedContextCoder([(h, w)], c, _wh([(h, w)]))          # no length given: 16384
        plain.encode(_dev(y.reshape(-1)), sd)
        assert plain.containers() == [want]


# ---- one ragged batch of mixed lengths --------------------------------------------------------------------------------------------
def test_mixed_lengths_in_one_batch_and_a_container_of_another_length(codec):
    shapes = [(h, w) for h, w, _ in MIXED]
    coder, ys, ss, sd, back = _ragged(codec, shapes, 192, MIXED_LENGTHS)
    wants = [sl.container(sh, S) for sh, S in zip(MIXED, MIXED_LENGTHS)]
    assert coder.enc_status.cpu().tolist() == [[0, len(b)] for b in wants]
    assert coder.containers() == wants
    assert coder.dec_status.cpu().tolist() == [[0, y.size] for y in ys] and torch.equal(back, _pack(ys))
    for im, sh, S in zip(coder.images, MIXED, MIXED_LENGTHS):
        assert (im.anchor_streams, im.nonanchor_streams) == sl.geometry(*sh, S)[1]
    # the same containers handed to a coder made for [1024, 16384, 1024]: image 2's header disagrees (bit 2), for that image alone
    other = codec.RaggedContextCoder(shapes, 192, _wh(shapes), stream_symbols=[1024, 16384, 1024])
    host = torch.zeros(other.slot_bytes, dtype=torch.uint8)
    for b, im in zip(wants, other.images):
        assert len(b) <= int(im.slot_bytes)
        host[int(im.slot_offset):int(im.slot_offset) + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
    out = torch.full_like(back, 0xEE)
    valid = torch.tensor([[0, len(b)] for b in wants], dtype=torch.int32).cuda()
    other.decode(out, sd, slots=host.cuda(), valid=valid)
    torch.cuda.synchronize()
    st = other.dec_status.cpu().tolist()
    assert [e for e, _ in st[:2]] == [0, 0] and st[2][0] & 4
    assert sl.ref_decode(wants[2], ss[2], 1024)[0] == -sl.V_HEADER
    views = other.views(out)
    assert np.array_equal(views[0].cpu().numpy(), ys[0]) and np.array_equal(views[1].cpu().numpy(), ys[1])
    assert not views[2].any()                                 # a rejected container leaves zeros


# ---- hostile containers at S = 1024 -------------------------------------------------------------------------------------------------
def _decode_pair(codec, blobs, shape, valid_bytes=None):
    """Two containers of `shape` at 1024 through one ragged decode: ([error, bytes] * 2, decoded latents)."""
    h, w, c = shape
    coder = codec.RaggedContextCoder([(h, w)] * 2, c, _wh([(h, w)] * 2), stream_symbols=1024)
    host = torch.zeros(coder.slot_bytes, dtype=torch.uint8)
    for b, im in zip(blobs, coder.images):
        host[int(im.slot_offset):int(im.slot_offset) + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
    valid = torch.tensor([[0, v] for v in (valid_bytes or [len(b) for b in blobs])], dtype=torch.int32).cuda()
    _, s = sl.latent(shape)
    out = torch.full((coder.latent_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    coder.decode(out, _pack([s, s]), slots=host.cuda(), valid=valid)
    torch.cuda.synchronize()
    return coder.dec_status.cpu().tolist(), [v.cpu().numpy() for v in coder.views(out)]


def test_hostile_containers_at_1024(codec):
    shape = (37, 37, 192)
    y, s = sl.latent(shape)
    good = sl.container(shape, 1024)
    _, _, lens = sl.fields(good)
    ns, fixed = lens.size, sl.HEADER + sl.TABLES + 4 * lens.size
    assert ns == 258
    # a length entry of cap(1024) + 2: above what a 1024-symbol stream can have, far below the 33024 of a 16384-symbol one.  Bit 5
    # either way — a decoder that bounded the entry by 33024 would still find the stream not ending where its length says — so this
    # case shows the verdict and its confinement, not which of the two bounds the device code uses
    entry = bytearray(good)
    entry[sl.HEADER + sl.TABLES + 4 * 100:sl.HEADER + sl.TABLES + 4 * 101] = (sl.cap(1024) + 2).to_bytes(4, "little")
    assert sl.cap(1024) + 2 < sl.cap(16384)
    st, lat = _decode_pair(codec, [good, bytes(entry)], shape)
    assert st[0] == [0, y.size] and np.array_equal(lat[0], y)
    assert st[1][0] & 32 and sl.ref_decode(bytes(entry), s, 1024)[0] == -sl.V_STREAM
    # a flipped payload byte: the stream it lies in (bit 5) or, where the stream still ends well, the checksum (bit 7)
    flipped = bytearray(good)
    flipped[fixed + int(lens[:130].sum()) + 300] ^= 0x10
    st, lat = _decode_pair(codec, [bytes(flipped), good], shape)
    rc = sl.ref_decode(bytes(flipped), s, 1024)[0]
    assert rc in (-sl.V_STREAM, -sl.V_CHECKSUM)
    assert st[0][0] & -rc and st[0][0] & ~(32 | 128) == 0
    assert st[1] == [0, y.size] and np.array_equal(lat[1], y)           # confined to its image
    # a short `valid`: the payload no longer fits (bit 4); shorter than the fixed part (bits 8 + 2)
    st, _ = _decode_pair(codec, [good, good], shape, valid_bytes=[len(good) - 10, fixed - 4])
    assert st[0][0] & 16 and sl.ref_decode(good[:len(good) - 10], s, 1024)[0] == -sl.V_PAYLOAD
    # (the full decoder reports 0x124: the parse stage's 0x104, and bit 5 from every stream, which finds a payload of 0 bytes)
    assert st[1][0] == 0x124 and sl.ref_decode(good[:fixed - 4], s, 1024)[0] == -sl.V_SHORT


# ---- a batch of more stream groups than the chip has compute units ------------------------------------------------------------------
def test_large_batch_of_short_streams(codec):
    """8 images of 64 x 64 x 192 at 1024 are 384 groups of 8 streams per set, against 256 CUs (one decoder workgroup per CU), and one
    image of 6 groups; then the same shapes at a batch of 1."""
    shapes = [(64, 64)] * 8 + [(20, 24)]
    assert [sum(sl.geometry(h, w, 192, 1024)[1]) for h, w in shapes[7:]] == [768, 90]
    coder, ys, ss, sd, back = _ragged(codec, shapes, 192, 1024, variants=list(range(9)))
    wants = [sl.container((h, w, 192), 1024, v) for v, (h, w) in enumerate(shapes)]
    assert coder.containers() == wants
    assert coder.dec_status.cpu().tolist() == [[0, y.size] for y in ys] and torch.equal(back, _pack(ys))
    # the uniform decoder over the eight: 384 groups per set as well
    y8, s8 = np.stack(ys[:8]), np.stack(ss[:8])
    uni = codec.ContextCoder(8, 64, 64, 192, *sl.image_wh((64, 64, 192)), stream_symbols=1024)
    uni.dec_status.fill_(-1)
    uni.encode(_dev(y8), _dev(s8))
    out = torch.full((8, 64, 64, 192), 0xEE, dtype=torch.uint8, device="cuda")
    uni.decode(out, _dev(s8))
    torch.cuda.synchronize()
    assert [uni.slots[i, :n].cpu().numpy().tobytes() for i, n in enumerate(uni.sizes())] == wants[:8]
    assert uni.dec_status.cpu().tolist() == [[0, y8[0].size]] * 8 and np.array_equal(out.cpu().numpy(), y8)
    for i in (0, 8):                                          # the same shapes alone
        one, y1, _, _, b1 = _ragged(codec, [shapes[i]], 192, 1024, variants=[i])
        assert one.containers() == [wants[i]] and one.dec_status.cpu().tolist() == [[0, y1[0].size]] and torch.equal(b1, _pack(y1))


# ---- capture into a graph -----------------------------------------------------------------------------------------------------------
def test_encode_and_decode_captured_in_one_graph_at_2048(codec):
    shapes = [(h, w) for h, w, _ in MIXED]
    coder = codec.RaggedContextCoder(shapes, 192, _wh(shapes), stream_symbols=2048)
    ys, ss = zip(*[sl.latent(sh) for sh in MIXED])
    yd, sd = _pack(ys), _pack(ss)
    back = torch.empty_like(yd)

    def enqueue():
        coder.encode(yd, sd)
        coder.decode(back, sd)
    enqueue()                                                  # warm-up: module load
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):            # one stream, no parallel branches
            enqueue()
    for variant in (1, 2):
        fy, fs = zip(*[sl.latent(sh, variant) for sh in MIXED])
        yd.copy_(_pack(fy))
        sd.copy_(_pack(fs))
        coder.slot_buffer.zero_()
        coder.enc_status.fill_(-1)
        coder.dec_status.fill_(-1)
        back.fill_(0xEE)
        graph.replay()
        torch.cuda.synchronize()
        assert coder.containers() == [sl.container(sh, 2048, variant) for sh in MIXED]
        assert coder.dec_status.cpu().tolist() == [[0, y.size] for y in fy] and torch.equal(back, yd)


# ---- the window decoder ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1024, 4096])
def test_window_decoder_at_short_lengths(codec, S):
    shapes = [(h, w) for h, w, _ in BIG]
    coder, ys, ss, sd, _ = _ragged(codec, shapes, 192, S)
    assert coder.containers() == [sl.container(sh, S) for sh in BIG]
    windows = [[(0, 3), (0, 5)], [(35, 2), (38, 2)], [(7, 1), (9, 1)], [(8, 1), (20, 1)], [(12, 9), (12, 16)], [(0, 37), (0, 40)]]
    for rows in windows:      # top, bottom, one row at an odd and at an even r0, a middle band, the whole image
        win = coder.window(rows)
        band = torch.full((win.band_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
        win.decode(band, sd)
        win.check()
        assert win.status.cpu().tolist() == [[0, int(im.symbols)] for im in win.images[:2]]
        host = band.cpu().numpy()
        for im, sh, y, (r0, rh), v in zip(win.images, BIG, ys, rows, win.views(band)):
            mask = sl.selected_mask(sh, S, tuple(im.first_stream), tuple(im.end_stream))
            want = np.where(mask, y, 0)[im.band_row0:im.band_row0 + im.band_rows]
            got = host[int(im.band_offset):int(im.band_offset) + int(im.band_bytes)].reshape(want.shape)
            assert np.array_equal(got, want), (rows, sh)                         # the selected streams' symbols, zero elsewhere
            assert np.array_equal(v.cpu().numpy(), y[r0:r0 + rh])                # the rows asked for are complete
            assert int(mask.sum()) == im.symbols
    # the band of a middle window is shorter than the same window's at 16384
    ref16 = codec.RaggedContextCoder(shapes, 192, _wh(shapes)).window([(12, 9), (12, 16)])
    win = coder.window([(12, 9), (12, 16)])
    assert all(a.band_rows <= b.band_rows for a, b in zip(win.images[:2], ref16.images[:2])) and win.selected_streams > 0
    if S == 1024:
        assert win.images[1].band_rows < ref16.images[1].band_rows
    # a flipped byte in a stream outside the window is neither read nor reported; inside, it is bit 5 for that image alone
    blob = sl.container(BIG[1], S)
    _, _, lens = sl.fields(blob)
    fixed = sl.HEADER + sl.TABLES + 4 * lens.size
    im = win.images[1]
    inside, outside = int(im.first_stream[0]), int(im.end_stream[0]) + 1
    assert outside < sl.geometry(*BIG[1], S)[1][0]
    for st, expect in ((outside, 0), (inside, 32)):
        bad = bytearray(blob)
        bad[fixed + int(lens[:st].sum()) + 200] ^= 0x20
        slots = coder.slot_buffer.clone()
        at = int(coder.images[1].slot_offset)
        slots[at:at + len(bad)] = _dev(np.frombuffer(bytes(bad), np.uint8))
        band = torch.full((win.band_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
        win.decode(band, sd, slots=slots, valid=coder.enc_status)
        torch.cuda.synchronize()
        got = win.status.cpu().tolist()
        assert got[0][0] == 0 and got[1][0] == expect, (st, got)
        if not expect:
            assert np.array_equal(win.views(band)[1].cpu().numpy(), ys[1][12:28])


# ---- the hyperprior codecs end to end ----------------------------------------------------------------------------------------------------
HYPER_SIZES = [(48, 48), (100, 36), (592, 592)]             # (width, height)


@pytest.mark.parametrize("use_gdn", [True, False], ids=["gdn", "plain"])
def test_ragged_hyperprior_codec_at_2048(codec, use_gdn):
    from simple_image_compression_network_amd import hyperprior
    rng = np.random.default_rng(592)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in HYPER_SIZES]
    base = hyperprior.RaggedHyperpriorCodec(HYPER_SIZES, seed=5, use_gdn=use_gdn)
    base.encode(base.main.pack([torch.from_numpy(x) for x in images]))
    want = base.decode().clone()
    base.check()
    short = hyperprior.RaggedHyperpriorCodec(HYPER_SIZES, seed=5, use_gdn=use_gdn, y_stream_symbols=2048)
    assert short.y_coder.stream_symbols == [2048] * 3 and base.y_coder.stream_symbols == [16384] * 3
    short.encode(short.main.pack([torch.from_numpy(x) for x in images]))
    b = short.archive()
    zy, zy0 = short.containers(), base.containers()
    assert [z for z, _ in zy] == [z for z, _ in zy0]                                  # the z containers are unchanged
    lat = short.main.shapes(3)
    y_host = [v.cpu().numpy() for v in short.main.views(3, short.y)]
    s_host = [v.cpu().numpy() for v in short.main.views(3, short.s)]
    for (_, yc), (_, yc0), (h, w, c), y, s, wh in zip(zy, zy0, lat, y_host, s_host, HYPER_SIZES):
        assert int(codec.parse_header(yc[:48]).stream_symbols) == 2048 and int(codec.parse_header(yc0[:48]).stream_symbols) == 16384
        assert yc == sl.ref_encode(y, s, 2048, wh)
        assert yc0 == sl.ref_encode(y, s, 16384, wh) == c_oracle.ctx_encode(y, s, wh)     # the reference held to the oracle on these latents
    other = hyperprior.RaggedHyperpriorCodec.from_archive(b, seed=5)                  # no length given: read from the y headers
    assert other.y_coder.stream_symbols == [2048] * 3 and other.use_gdn == use_gdn and other.sizes == HYPER_SIZES
    got = other.decode(archive=b)
    other.check()
    torch.cuda.synchronize()
    assert torch.equal(got, want), "the reconstruction depends on the stream length"   # the coder is lossless: pixels cannot depend on S
    full = [v.cpu().numpy() for v in other.main.crop_views(other.main.cropped(got))]
    sel, rois = [0, 2], [(5, 9, 30, 20), (168, 168, 256, 256)]
    part = hyperprior.RaggedHyperpriorCodec.from_archive(b, seed=5, images=sel)
    assert part.y_coder.stream_symbols == [2048] * 2
    pix = part.decode(archive=b, images=sel, rois=rois)
    part.check()
    for v, i, (x0, y0, w, h) in zip(part.roi_views(pix), sel, rois):
        assert np.array_equal(v.cpu().numpy(), full[i][y0:y0 + h, x0:x0 + w])
    # the window the 256 x 256 detail selects is finer than at 16384
    base_roi = base.roi([None, None, rois[1]])
    assert part._last_roi.window.images[1].band_rows <= base_roi.window.images[2].band_rows


def test_uniform_hyperprior_codec_at_2048(codec):
    from simple_image_compression_network_amd import hyperprior
    rng = np.random.default_rng(176)
    x = _dev(rng.integers(0, 256, (2, 144, 176, 3), dtype=np.uint8))
    base = hyperprior.HyperpriorCodec(176, 144, 2, seed=3)
    short = hyperprior.HyperpriorCodec(176, 144, 2, seed=3, y_stream_symbols=2048)
    assert short.y_coder.stream_symbols == 2048 and base.y_coder.stream_symbols == 16384
    outs = []
    for hc in (base, short):
        hc.encode(x)
        out = torch.empty((2,) + tuple(hc.main.descs[-1].out_shape), dtype=torch.uint8, device="cuda")
        hc.decode(out)
        hc.check()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    zs = base.z_coder.sizes()
    assert zs == short.z_coder.sizes() and all(torch.equal(base.z_coder.slots[i, :n], short.z_coder.slots[i, :n]) for i, n in enumerate(zs))
    y, s = short.y.cpu().numpy(), short.s.cpu().numpy()
    for i, n in enumerate(short.y_coder.sizes()):
        assert short.y_coder.slots[i, :n].cpu().numpy().tobytes() == sl.ref_encode(y[i], s[i], 2048, (176, 144))
        n0 = base.y_coder.sizes()[i]                          # the reference held to the oracle on these latents, at 16384
        assert base.y_coder.slots[i, :n0].cpu().numpy().tobytes() == sl.ref_encode(y[i], s[i], 16384, (176, 144)) == c_oracle.ctx_encode(y[i], s[i], (176, 144))
