"""GPU checks of the entropy coders at their edges (run with -m gpu on an MI355X).  Everything is byte equality against the C oracle
(oracle/sicn_codec_oracle.c, oracle/sicn_hyper_oracle.c) plus decode(encode(x)) == x; inputs and the oracle's containers come from
tests/codec_edge_cases.py, whose CPU half is tests/test_codec_edges.py.

  * the context coder (mode 4) over degenerate class statistics x stream geometry, in batches of three different images;
  * rANS-W and rANS-WC streams at the format's maximum rate of 12 bits per symbol: 12288 + 128 words through the 4096-word LDS ring
    (three wraps; the flush margin of the encoders and the refill bound of the decoders are exact), in every decoder form;
  * everything the mode-4 decoder says it rejects, with the neighbours of the bad container decoding exactly;
  * guard bands around every buffer of the context coder, and the argument checks of its two C entry points."""
import ctypes
import struct

import numpy as np
import pytest

import codec_edge_cases as ce
from oracle import c_oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL, ENOSPC = -22, -28
GUARD = 4096
PATTERN = 0xA5


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import codec as _codec
    return _codec


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()   # (the cached cases are read-only arrays)


def _ctx_equals_oracle_and_round_trips(codec, y, s, want, wh):
    """One ContextCoder run over the batch (y, s): containers, sizes, both status arrays, the decoded latent."""
    n_img, shape = y.shape[0], y.shape[1:]
    yd, sd = _dev(y), _dev(s)
    coder = codec.ContextCoder(n_img, *shape, image_width=wh[0], image_height=wh[1])
    coder.enc_status.fill_(-1)                                      # a status word nobody wrote does not read as "no error"
    coder.dec_status.fill_(-1)
    coder.encode(yd, sd)
    back = torch.full_like(yd, 0xEE)
    coder.decode(back, sd)
    torch.cuda.synchronize()
    enc, dec = coder.enc_status.cpu().numpy(), coder.dec_status.cpu().numpy()
    assert not enc[:, 0].any(), f"encoder status {enc[:, 0]}"
    assert coder.sizes() == [len(b) for b in want]
    host = coder.slots.cpu().numpy()
    for i, b in enumerate(want):
        assert host[i, :len(b)].tobytes() == b, f"image {i}: container differs from the oracle's"
    assert not dec[:, 0].any(), f"decoder status {dec[:, 0]}"
    assert (dec[:, 1] == y[0].size).all()
    assert torch.equal(back, yd)
    return coder


# ---- the context coder: distribution x geometry --------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", range(len(ce.CTX_BATCHES)), ids=["+".join(b) for b in ce.CTX_BATCHES])
@pytest.mark.parametrize("shape", ce.CTX_BIG + ce.CTX_SMALL, ids=lambda sh: "x".join(map(str, sh)))
def test_ctx_matrix_equals_oracle_and_round_trips(codec, shape, batch):
    """One class only, f = 4096, f = 1 beside 4095, tied maxima in the walk of k_ctx_tables (towards both sides); a set of exactly
    16384 symbols, a last stream of 4 symbols ((1, 8193, 4): one live lane), 18 streams per image ((37, 37, 192): the last workgroup
    of k_ctx_encode half empty, 9 per set: the second one of k_ctx_decode with one wave), no non-anchors at all ((1, 1, 4))."""
    y, s, want = ce.ctx_case(shape, batch)
    _ctx_equals_oracle_and_round_trips(codec, y, s, want, (shape[1] * 16, shape[0] * 16))


# ---- streams at the format's maximum rate ------------------------------------------------------------------------------------
def _small(rng, shape):
    x = np.minimum(rng.geometric(0.2, shape), 127)
    x[rng.random(shape) < 0.5] = 0
    return x.astype(np.uint8)


@pytest.mark.parametrize("name", list(ce.RATE3))
def test_max_rate_mode3_streams(codec, name):
    """Hot streams of exactly 1.5 ss + 256 bytes (asserted from the oracle's container before anything runs on the GPU) at the head, in
    the middle and at the end of the image, the short tail hot too: the asynchronous pair at the case's stream length (65 streams:
    the latency form of the decoder; 1301: the self form with two tables; 2050: the scan form), the synchronous pair, and the ragged
    coder with the same image next to two small ones."""
    n, ss, hot = ce.RATE3[name]
    ce.assert_rate3_is_at_the_bound(name)
    lat, want, _ = ce.rate3_case(name)
    dev = _dev(lat)
    # the asynchronous pair
    coder = codec.LatentCoder(1, 1, 1, n, stream_symbols=ss)
    coder.enc_status.fill_(-1)
    coder.dec_status.fill_(-1)
    coder.encode(dev[None])
    back = torch.full_like(dev[None], 0xEE)
    coder.decode(back)
    torch.cuda.synchronize()
    assert coder.enc_status.cpu().tolist() == [[0, len(want)]] and coder.dec_status.cpu().tolist() == [[0, n]]
    assert coder.slots[0, :len(want)].cpu().numpy().tobytes() == want
    assert torch.equal(back[0], dev)
    # the synchronous pair: the encoder writes the format's default length, the decoder reads the length from the header
    blob = codec.encode_latent(dev, 0, 0, codec.RANSW).cpu().numpy().tobytes()
    want16 = want if ss == 16384 else c_oracle.codec_encode(lat, (0, 0), 3)
    assert blob == want16
    for b, length in ((want, ss), (want16, 16384))[:1 if ss == 16384 else 2]:
        got, info = codec.decode_latent(_dev(np.frombuffer(b, np.uint8)))
        assert torch.equal(got, dev) and int(info.stream_symbols) == length
    slots, sizes = codec.encode_latents(dev[None], 0, 0)
    assert sizes == [len(want16)] and slots[0, :sizes[0]].cpu().numpy().tobytes() == want16
    got, _ = codec.decode_latents(slots, sizes)
    assert torch.equal(got[0], dev)
    if -(-n // ss) > 2048:                                          # the ragged coder has the self form only
        return
    rng = np.random.default_rng(n + 1)
    shapes, lengths = [(2, 7), (1, n), (3, 5)], [8192, ss, 8192]
    lats = [_small(rng, (2, 7, 1)), lat.reshape(1, n, 1), _small(rng, (3, 5, 1))]
    wants = [c_oracle.codec_encode(x, (0, 0), 3, stream_symbols=sl) for x, sl in zip(lats, lengths)]
    assert wants[1][ce.HEADER:] == want[ce.HEADER:]                 # the same table, lengths and streams: still at the bound
    ragged = codec.RaggedLatentCoder(shapes, 1, None, lengths)
    ragged.enc_status.fill_(-1)
    ragged.dec_status.fill_(-1)
    packed = _dev(np.concatenate([x.reshape(-1) for x in lats]))
    ragged.encode(packed)
    back = torch.full_like(packed, 0xEE)
    ragged.decode(back)
    torch.cuda.synchronize()
    assert ragged.enc_status.cpu().tolist() == [[0, len(b)] for b in wants]
    assert ragged.containers() == wants
    assert ragged.dec_status.cpu().tolist() == [[0, x.size] for x in lats]
    assert torch.equal(back, packed)


@pytest.mark.parametrize("h", [200, 201])
def test_max_rate_mode4_streams(codec, h):
    """k_ctx_encode / k_ctx_decode carry their own copies of the step loops: streams of up to 24832 bytes (asserted from the oracle's
    containers first) at both ends of either set, hot on the anchors, on the non-anchors, on both; at h = 201 the hot band is split
    between the last two streams of a set."""
    ce.assert_rate4_is_near_the_bound(h)
    y, s, want = ce.rate4_case(h)
    _ctx_equals_oracle_and_round_trips(codec, y, s, want, (37 * 16, h * 16))


# ---- what the mode-4 decoder must reject --------------------------------------------------------------------------------------
HOSTILE_SHAPE = (9, 10, 192)            # 8640 + 8640 symbols: two streams
HOSTILE_FIXED = ce.CTX_LENS + 4 * 2     # header, tables, length table


def _put32(buf, off, v):
    buf[off:off + 4] = np.frombuffer(struct.pack("<I", v & 0xFFFFFFFF), np.uint8)


def _hostile_cases(good, size):
    """[(name, container bytes of image 1 (whole slot), valid bytes, does the oracle see it)] from the good slot of image 1.

    Why no case can make the decoder touch memory outside the slot, the workspace and the latent (csrc/sicn_codec_ctx.inc):
      * k_ctx_parse reads bytes 0..47 of the slot, and only if valid >= fixed (4152 here); valid itself is clamped to the slot size.
        The payload field is accepted only if it is <= valid - fixed, else the streams get a payload of 0 bytes.
      * k_ctx_tables reads the 4096 table bytes (inside the fixed part, skipped when parse said 0x100); a row whose sum is neither
        0 nor 4096 is replaced by zeros, so every cumulative value is <= 4096.  Its slot-table walk indexes cum[cls][sy + 1] with
        sy <= 127 because cum[cls][128] = 0xFFFF stops it; its stores go to workspace addresses that depend on class and lane only.
      * k_ctx_scan reads the 8 bytes of the length table (inside the fixed part, skipped on 0x100), counts an entry above 33024 as 0, so the
        32-bit sums cannot wrap, and writes offsets[0..2].
      * k_ctx_decode refuses a stream unless 256 <= len <= 33024, len and off even and off + len <= payload bytes (a 64-bit sum):
        every payload read is below fixed + payload <= valid.  The ring is indexed modulo 4096, the slot table with class * 4096 + 12
        bits, the frequency table with class * 128 + 7 bits; classes are masked to 4 bits.  Latent loads and stores use addresses
        made of the CALLER's W, H, C only — no header field, no decoded value.
      * k_stats and k_ctx_finish read the latent and the workspace."""
    head, tables, lens = ce.ctx_container_fields(good[:size].tobytes())
    pb = int(lens.sum())
    assert lens.size == 2 and pb == size - HOSTILE_FIXED
    cases = []

    def add(name, patch=None, valid=size, oracle_sees=True):
        c = good.copy()
        if patch:
            patch(c)
        cases.append((name, c, valid, oracle_sees))

    def lens_patch(entries):
        def f(c):
            for k, v in enumerate(entries):
                _put32(c, ce.CTX_LENS + 4 * k, v)
        return f
    g0, g1 = int(lens[0]), int(lens[1])
    for k, entries in enumerate([[0xFFFF0000, (pb - 0xFFFF0000) % (1 << 32)], [0xFFFFFFFF, 1 + pb], [pb + 2, 0xFFFFFFFE], [g0, 0x40000000],
                                 [0x7FFFFFF0, 0x7FFFFFF0], [g0 + 2, g1 - 2]]):
        add(f"lengths-{k}", lens_patch(entries))
    used = int(np.argmax((tables > 0).sum(axis=1)))                  # the class with the most symbols in use
    row = tables[used].astype(np.int64)
    assert row.sum() == 4096
    top = np.argsort(-row, kind="stable")[:2]
    assert row[top[0]] > row[top[1]] > 0

    def row_patch(new):
        def f(c):
            c[ce.HEADER + 256 * used:ce.HEADER + 256 * (used + 1)] = np.asarray(new, "<u2").view(np.uint8)
        return f
    minus = row.copy(); minus[top[0]] -= 1
    swapped = row.copy(); swapped[top] = row[top[::-1]]
    add("row-sum-4095", row_patch(minus))
    add("row-sum-8192", row_patch(2 * row))
    add("row-zeroed", row_patch(0 * row))
    add("row-two-exchanged", row_patch(swapped))
    w, h, c_, n = (int(v) for v in head[4:8])
    for name, dwords in [("magic", {0: int(head[0]) ^ 1}), ("mode-3", {1: 1 | (3 << 16)}), ("version", {1: 2 | (4 << 16)}), ("w", {4: w + 1}),
                         ("h", {5: h + 1}), ("w-h-swapped", {4: h, 5: w}), ("c", {6: c_ + 4}), ("n", {7: n + 1}), ("n-streams", {8: 3}),
                         ("stream-symbols", {9: 8192})]:
        add("header-" + name, lambda c, d=dwords: [_put32(c, 4 * k, v) for k, v in d.items()])
    add("payload-field-beyond-valid", lambda c: _put32(c, 40, pb + 2))
    add("valid-40", None, 40)
    add("valid-fixed-minus-1", None, HOSTILE_FIXED - 1)
    return cases


def test_ctx_decoder_rejects_and_isolates(codec):
    rng = np.random.default_rng(44)
    s = rng.integers(0, 128, (3,) + HOSTILE_SHAPE, dtype=np.uint8)
    y = np.minimum((rng.exponential(1.0, s.shape) * (s / 8 + 0.5)).astype(np.int64), 127).astype(np.uint8)
    yd, sd = _dev(y), _dev(s)
    coder = codec.ContextCoder(3, *HOSTILE_SHAPE, image_width=160, image_height=144)
    coder.encode(yd, sd)
    coder.check()
    enc = coder.enc_status.clone()
    sizes = coder.sizes()
    good = coder.slots.cpu().numpy().copy()
    assert good[1, :sizes[1]].tobytes() == c_oracle.ctx_encode(y[1], s[1], (160, 144))
    for name, container, valid, oracle_sees in _hostile_cases(good[1], sizes[1]):
        slots = good.copy()
        slots[1] = container
        slots_d = _dev(slots)
        valid_d = enc.clone()
        valid_d[1, 1] = valid
        outs = []
        for fill in (0x00, 0xEE):
            back = torch.full_like(yd, fill)
            coder.dec_status.fill_(-1)
            coder.decode(back, sd, slots=slots_d, valid=valid_d)
            torch.cuda.synchronize()
            st = coder.dec_status.cpu().numpy()
            assert st[1, 0] != 0 and st[0, 0] == 0 and st[2, 0] == 0, (name, st)
            assert torch.equal(back[0], yd[0]) and torch.equal(back[2], yd[2]), name
            outs.append(back[1].cpu().numpy())
        assert np.array_equal(outs[0], outs[1]), f"{name}: the rejected image depends on what the buffer held"
        if oracle_sees:
            with pytest.raises(RuntimeError):
                c_oracle.ctx_decode(container[:valid].tobytes(), s[1])
    back = torch.full_like(yd, 0xEE)
    coder.decode(back, sd, slots=_dev(good), valid=enc)
    coder.check()
    assert torch.equal(back, yd)


# ---- buffers and arguments --------------------------------------------------------------------------------------------------------
class _CtxCall:
    """The two C entry points of the context coder on buffers with guard bands on either side."""

    def __init__(self, shape, n_img=3):
        from simple_image_compression_network_amd import _lib
        self.L = _lib.lib()
        self.shape, self.n_img = shape, n_img
        h, w, c = shape
        self.n = h * w * c
        self.max_bytes = int(self.L.sicn_codec_ctx_max_bytes(w, h, c))
        self.slot = (self.max_bytes + 255) // 256 * 256
        self.ws_bytes = int(self.L.sicn_codec_ctx_workspace_bytes(w, h, c, n_img))
        self.sizes = {"slots": n_img * self.slot, "ws": self.ws_bytes, "back": n_img * self.n, "enc": 8 * n_img, "dec": 8 * n_img}
        self.buf = {k: torch.full((GUARD + v + GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for k, v in self.sizes.items()}
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ptr(self, name, off=0):
        return ctypes.c_void_p(self.buf[name].data_ptr() + GUARD + off)

    def inner(self, name):
        return self.buf[name][GUARD:GUARD + self.sizes[name]]

    def guards_intact(self):
        torch.cuda.synchronize()
        for name, t in self.buf.items():
            hst = t.cpu().numpy()
            assert (hst[:GUARD] == PATTERN).all() and (hst[GUARD + self.sizes[name]:] == PATTERN).all(), f"guard band of `{name}` was written"

    def untouched(self):
        torch.cuda.synchronize()
        for name, t in self.buf.items():
            assert (t.cpu().numpy() == PATTERN).all(), f"`{name}` was written"

    def encode(self, y_ptr, s_ptr, **kw):
        h, w, c = self.shape
        a = dict(lat=ctypes.c_void_p(y_ptr), sc=ctypes.c_void_p(s_ptr), n_img=self.n_img, w=w, h=h, c=c, out=self.ptr("slots"), slot=self.slot,
                 status=self.ptr("enc"), ws=self.ptr("ws"), ws_bytes=self.ws_bytes)
        a.update(kw)
        return self.L.sicn_codec_ctx_encode_batch_async(a["lat"], a["sc"], a["n_img"], a["w"], a["h"], a["c"], 16 * w, 16 * h, a["out"], a["slot"],
                                                        a["status"], a["ws"], a["ws_bytes"], self.stream)

    def decode(self, s_ptr, **kw):
        h, w, c = self.shape
        a = dict(cont=self.ptr("slots"), slot=self.slot, valid=self.ptr("enc"), sc=ctypes.c_void_p(s_ptr), n_img=self.n_img, w=w, h=h, c=c,
                 lat=self.ptr("back"), status=self.ptr("dec"), ws=self.ptr("ws"), ws_bytes=self.ws_bytes)
        a.update(kw)
        return self.L.sicn_codec_ctx_decode_batch_async(a["cont"], a["slot"], a["valid"], a["sc"], a["n_img"], a["w"], a["h"], a["c"], a["lat"],
                                                        a["status"], a["ws"], a["ws_bytes"], self.stream)


@pytest.mark.parametrize("shape", [(37, 37, 192), (1, 8193, 4)], ids=lambda sh: "x".join(map(str, sh)))
def test_ctx_stays_inside_its_buffers(codec, shape):
    """Slots, workspace, latents and both status arrays between guard bands: every guard byte intact after the encode and after the
    decode.  The uniform contents give the largest containers (238 KB each at (37, 37, 192))."""
    y, s, want = ce.ctx_case(shape, 1)
    yd, sd = _dev(y), _dev(s)
    call = _CtxCall(shape)
    assert call.encode(yd.data_ptr(), sd.data_ptr()) == 0
    call.guards_intact()
    enc = call.inner("enc").cpu().numpy().view("<i4").reshape(3, 2)
    assert enc.tolist() == [[0, len(b)] for b in want]
    host = call.inner("slots").cpu().numpy().reshape(3, call.slot)
    for i, b in enumerate(want):
        assert host[i, :len(b)].tobytes() == b, f"image {i}: container differs from the oracle's"
    assert call.decode(sd.data_ptr()) == 0
    call.guards_intact()
    dec = call.inner("dec").cpu().numpy().view("<i4").reshape(3, 2)
    assert dec.tolist() == [[0, call.n]] * 3
    assert np.array_equal(call.inner("back").cpu().numpy().reshape(y.shape), y)
    assert np.array_equal(call.inner("slots").cpu().numpy().reshape(3, call.slot), host)      # the decoder writes no slot byte


def test_ctx_argument_checks_return_without_launching(codec):
    """The codes the two entry points return today, and that nothing was enqueued: every buffer still holds its fill pattern."""
    shape = (37, 37, 192)
    h, w, c = shape
    y, s, _ = ce.ctx_case(shape, 1)
    yd, sd = _dev(y), _dev(s)
    lat, sc = yd.data_ptr(), sd.data_ptr()
    call = _CtxCall(shape)
    null = ctypes.c_void_p(None)
    enc_cases = {
        "lat_c % 4": (dict(c=190), EINVAL), "n == 0": (dict(w=0), EINVAL), "n_images > 65535": (dict(n_img=65536), EINVAL),
        "latents + 1": (dict(lat=ctypes.c_void_p(lat + 1)), EINVAL), "scales + 1": (dict(sc=ctypes.c_void_p(sc + 1)), EINVAL),
        "latents + 2": (dict(lat=ctypes.c_void_p(lat + 2)), EINVAL),
        "odd slot": (dict(slot=call.max_bytes + 1), ENOSPC), "slot 1 short": (dict(slot=call.max_bytes - 1), ENOSPC),
        "slot 2 short": (dict(slot=call.max_bytes - 2), ENOSPC), "workspace 1 short": (dict(ws_bytes=call.ws_bytes - 1), ENOSPC),
        "null latents": (dict(lat=null), EINVAL), "null scales": (dict(sc=null), EINVAL), "null out": (dict(out=null), EINVAL),
        "null status": (dict(status=null), EINVAL), "null workspace": (dict(ws=null), ENOSPC), "no images": (dict(n_img=0), 0),
    }
    for name, (kw, code) in enc_cases.items():
        assert call.encode(lat, sc, **kw) == code, f"encode, {name}"
    assert call.max_bytes % 2 == 0 and call.encode(lat, sc, slot=call.max_bytes, ws_bytes=call.ws_bytes - 1) == ENOSPC   # the slot passes at exactly max_bytes
    dec_cases = {
        "lat_c % 4": (dict(c=190), EINVAL), "n == 0": (dict(h=0), EINVAL), "n_images > 65535": (dict(n_img=65536), EINVAL),
        "latents + 1": (dict(lat=call.ptr("back", 1)), EINVAL), "scales + 1": (dict(sc=ctypes.c_void_p(sc + 1)), EINVAL),
        "odd slot": (dict(slot=call.slot - 1), EINVAL), "workspace 1 short": (dict(ws_bytes=call.ws_bytes - 1), ENOSPC),
        "null containers": (dict(cont=null), EINVAL), "null scales": (dict(sc=null), EINVAL), "null latents": (dict(lat=null), EINVAL),
        "null status": (dict(status=null), EINVAL), "null workspace": (dict(ws=null), ENOSPC), "no images": (dict(n_img=0), 0),
    }
    for name, (kw, code) in dec_cases.items():
        assert call.decode(sc, **kw) == code, f"decode, {name}"
    call.untouched()
