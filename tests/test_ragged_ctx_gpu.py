"""GPU checks of the ragged context coder (include/sicn_ragged_ctx.h, codec.RaggedContextCoder): n latents of n different shapes,
each with its scale map, in a fixed number of launches.  Everything is byte equality against oracle.c_oracle.ctx_encode / ctx_decode
per image; the inputs are those of tests/codec_edge_cases.py."""
import ctypes
import functools

import numpy as np
import pytest

import codec_edge_cases as ce
from oracle import c_oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL, ENOSPC = -22, -28
GUARD = 4096
PATTERN = 0xA5
# lat_c -> [(lat_h, lat_w)].  C = 4: a set of exactly 16384 symbols; 2 + 1 streams, the last anchor stream 4 symbols long; no non-anchors;
# image starts at 4-byte, not 16-byte, multiples.  C = 192: 9 + 9 streams (groups of 4 and of 8 leave a remainder) beside 1 + 0 and 2 + 2.
BATCHES = {4: [(64, 128), (2, 2), (3, 3), (1, 1), (1, 8193), (1, 1)],
           8: [(5, 1), (1, 5), (2, 3), (1, 1)],
           192: [(37, 37), (1, 1), (3, 5), (12, 16), (2, 7), (1, 2), (2, 1)]}
CONTENTS = list(ce.CTX_CONTENTS)


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import codec as _codec
    return _codec


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _wh(shapes):
    return [(16 * w, 16 * h) for h, w in shapes]


@functools.lru_cache(maxsize=None)
def _case(lat_c, rot):
    """([y], [s], [oracle container]) of a batch with content (i + rot) % 10 in image i; computed once, never modified."""
    shapes = BATCHES[lat_c]
    rng = np.random.default_rng([lat_c, rot])
    ys, ss = zip(*[ce.CTX_CONTENTS[CONTENTS[(i + rot) % len(CONTENTS)]]((h, w, lat_c), rng) for i, (h, w) in enumerate(shapes)])
    for a in ys + ss:
        a.setflags(write=False)
    return ys, ss, [c_oracle.ctx_encode(y, s, wh) for y, s, wh in zip(ys, ss, _wh(shapes))]


def _pack(arrays):
    return _dev(np.concatenate([a.reshape(-1) for a in arrays]))


def _round_trip(codec, shapes, lat_c, ys, ss, wants, uniform=True):
    """Encode + decode of one batch: containers, sizes, both status arrays and the decoded latents against the oracle; with `uniform`
    also against ContextCoder(1, ...) per image, in both directions.  Returns the coder."""
    coder = codec.RaggedContextCoder(shapes, lat_c, _wh(shapes))
    coder.enc_status.fill_(-1)                                      # a status word nobody wrote does not read as "no error"
    coder.dec_status.fill_(-1)
    yd, sd = _pack(ys), _pack(ss)
    coder.encode(yd, sd)
    back = torch.full_like(yd, 0xEE)
    coder.decode(back, sd)
    torch.cuda.synchronize()
    assert coder.enc_status.cpu().tolist() == [[0, len(b)] for b in wants]
    assert coder.sizes() == [len(b) for b in wants]
    got = coder.containers()
    for i, (a, b) in enumerate(zip(got, wants)):
        assert a == b, f"image {i} {shapes[i]}: container differs from the oracle's"
    assert coder.dec_status.cpu().tolist() == [[0, y.size] for y in ys]
    assert torch.equal(back, yd)
    for i, (v, y) in enumerate(zip(coder.views(back), ys)):
        assert np.array_equal(v.cpu().numpy(), y), f"image {i}"
    if uniform:
        for i, ((h, w), y, s, want, wh, slot) in enumerate(zip(shapes, ys, ss, wants, _wh(shapes), coder.slots())):
            one = codec.ContextCoder(1, h, w, lat_c, *wh)
            y1, s1 = _dev(y[None]), _dev(s[None])
            one.encode(y1, s1)
            torch.cuda.synchronize()
            assert one.sizes() == [len(want)] and one.slots[0, :len(want)].cpu().numpy().tobytes() == want, f"image {i}"
            ext = torch.zeros_like(one.slots)                        # our container, through the uniform decoder
            ext[0, :min(one.slot, slot.numel())] = slot[:min(one.slot, slot.numel())]
            out = torch.full_like(y1, 0xEE)
            one.decode(out, s1, slots=ext, valid=coder.enc_status[i:i + 1])
            one.check()
            assert torch.equal(out, y1), f"image {i}: our container through sicn_codec_ctx_decode_batch_async"
    return coder


@pytest.mark.parametrize("rot", range(len(CONTENTS)))
@pytest.mark.parametrize("lat_c", sorted(BATCHES))
def test_batches_equal_oracle_uniform_coder_and_round_trip(codec, lat_c, rot):
    ys, ss, wants = _case(lat_c, rot)
    _round_trip(codec, BATCHES[lat_c], lat_c, ys, ss, wants)


@pytest.mark.parametrize("lat_c", sorted(BATCHES))
def test_oracle_made_containers_decode_here(codec, lat_c):
    ys, ss, wants = _case(lat_c, 3)
    for y, s, b in zip(ys, ss, wants):
        assert np.array_equal(c_oracle.ctx_decode(b, s)[0], y)       # the oracle round-trips every shape
    coder = codec.RaggedContextCoder.for_containers(wants)
    assert coder.shapes == BATCHES[lat_c] and coder.image_sizes == _wh(BATCHES[lat_c])
    back = torch.full((coder.latent_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    coder.decode(back, _pack(ss))
    coder.check()
    assert torch.equal(back, _pack(ys))


def test_permuting_a_batch_permutes_the_containers(codec):
    ys, ss, wants = _case(192, 0)
    perm = [4, 0, 6, 2, 1, 5, 3]
    shapes = [BATCHES[192][i] for i in perm]
    coder = _round_trip(codec, shapes, 192, [ys[i] for i in perm], [ss[i] for i in perm], [wants[i] for i in perm], uniform=False)
    assert coder.containers() == [wants[i] for i in perm]


def test_full_rate_streams_as_one_batch(codec):
    """The six images of rate4_case(200) and rate4_case(201): streams near the 24832 bytes a stream can have, at both ends of either set."""
    ys, ss, wants, shapes = [], [], [], []
    for h in (200, 201):
        ce.assert_rate4_is_near_the_bound(h)
        y, s, want = ce.rate4_case(h)
        ys += list(y); ss += list(s); wants += want; shapes += [(h, 37)] * 3
    _round_trip(codec, shapes, 192, ys, ss, wants, uniform=False)


def test_seventy_small_images(codec):
    small = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (2, 3)]
    shapes = [small[i % len(small)] for i in range(70)]
    rng = np.random.default_rng(70)
    ys, ss = zip(*[ce.CTX_CONTENTS[CONTENTS[i % len(CONTENTS)]]((h, w, 4), rng) for i, (h, w) in enumerate(shapes)])
    wants = [c_oracle.ctx_encode(y, s, wh) for y, s, wh in zip(ys, ss, _wh(shapes))]
    _round_trip(codec, shapes, 4, ys, ss, wants, uniform=False)


@pytest.mark.parametrize("where", ["latent", "scale"])
def test_a_symbol_of_128_or_more_is_reported_for_its_image_only(codec, where):
    shapes, lat_c, bad = BATCHES[192], 192, 3
    ys, ss, wants = _case(lat_c, 5)
    ys, ss = [np.array(y) for y in ys], [np.array(s) for s in ss]
    (ys if where == "latent" else ss)[bad].reshape(-1)[1234] = 128
    coder = codec.RaggedContextCoder(shapes, lat_c, _wh(shapes))
    coder.enc_status.fill_(-1)
    coder.encode(_pack(ys), _pack(ss))
    torch.cuda.synchronize()
    st = coder.enc_status.cpu().tolist()
    assert [e for e, _ in st] == [1 if i == bad else 0 for i in range(len(shapes))]
    host = coder.slot_buffer.cpu().numpy()
    for i, (im, want) in enumerate(zip(coder.images, wants)):
        if i != bad:
            assert st[i][1] == len(want) and host[int(im.slot_offset):int(im.slot_offset) + len(want)].tobytes() == want, f"image {i}"
    with pytest.raises(RuntimeError) as e:
        coder.check()
    assert e.value.image == bad


# ---- what the decoder must reject: one damaged container in one slot of a batch -----------------------------------------------------
HOSTILE = ["lengths-2", "row-two-exchanged", "header-n-streams", "payload-field-beyond-valid", "valid-40", "valid-fixed-minus-1"]


@pytest.fixture(scope="module")
def hostile(codec):
    """A good batch around an image of test_codec_edges_gpu's hostile shape, and that module's damaged versions of its container."""
    import test_codec_edges_gpu as edges
    lat_c, bad = 192, 2
    shapes = [(3, 5), (12, 16), edges.HOSTILE_SHAPE[:2], (1, 1), (2, 7)]
    rng = np.random.default_rng(45)
    ss = [rng.integers(0, 128, (h, w, lat_c), dtype=np.uint8) for h, w in shapes]
    ys = [np.minimum((rng.exponential(1.0, s.shape) * (s / 8 + 0.5)).astype(np.int64), 127).astype(np.uint8) for s in ss]
    coder = codec.RaggedContextCoder(shapes, lat_c, _wh(shapes))
    coder.encode(_pack(ys), _pack(ss))
    coder.check()
    size = coder.sizes()[bad]
    good = coder.slots()[bad].cpu().numpy().copy()
    assert good[:size].tobytes() == c_oracle.ctx_encode(ys[bad], ss[bad], _wh(shapes)[bad])
    cases = {name: (c, valid) for name, c, valid, _ in edges._hostile_cases(good, size)}
    return coder, bad, ys, ss, cases


@pytest.mark.parametrize("name", HOSTILE)
def test_a_damaged_container_is_rejected_and_isolated(hostile, name):
    coder, bad, ys, ss, cases = hostile
    container, valid = cases[name]
    slots = coder.slot_buffer.clone()
    coder.slots(slots)[bad].copy_(_dev(container))
    valid_d = coder.enc_status.clone()
    valid_d[bad, 1] = valid
    sd, yd = _pack(ss), _pack(ys)
    outs = []
    for fill in (0x00, 0xA5):
        back = torch.full_like(yd, fill)
        coder.dec_status.fill_(-1)
        coder.decode(back, sd, slots=slots, valid=valid_d)
        torch.cuda.synchronize()
        st = coder.dec_status.cpu().numpy()
        assert st[bad, 0] != 0 and not np.delete(st[:, 0], bad).any(), (name, st)
        views = coder.views(back)
        for i, y in enumerate(ys):
            if i != bad:
                assert np.array_equal(views[i].cpu().numpy(), y), f"{name}: neighbour {i}"
        outs.append(views[bad].cpu().numpy())
    assert np.array_equal(outs[0], outs[1]), f"{name}: the rejected image depends on what the buffer held"
    back = torch.full_like(yd, 0xEE)                                 # the coder is unharmed: its own slots still decode
    coder.decode(back, sd)
    coder.check()
    assert torch.equal(back, yd)


# ---- buffers and arguments: the C entry points on buffers between guard bands -------------------------------------------------------
class _Call:
    def __init__(self, shapes, lat_c):
        from simple_image_compression_network_amd import _lib
        self.L = _lib.lib()
        n = len(shapes)
        u32 = ctypes.c_uint32 * n
        self.images = (_lib.RaggedCtxImage * n)()
        totals = (ctypes.c_uint64 * 3)()
        lw, lh = u32(*[w for _, w in shapes]), u32(*[h for h, _ in shapes])
        assert self.L.sicn_ragged_ctx_layout(lw, lh, lat_c, n, self.images, totals) == 0
        iw, ih = u32(*[16 * w for _, w in shapes]), u32(*[16 * h for h, _ in shapes])
        self.h = ctypes.c_void_p()
        assert self.L.sicn_ragged_ctx_coder_create(lw, lh, lat_c, iw, ih, n, ctypes.byref(self.h)) == 0
        self.ws_bytes = int(self.L.sicn_ragged_ctx_coder_workspace_bytes(self.h))
        assert self.ws_bytes == int(totals[2])
        self.sizes = {"lat": int(totals[0]), "scale": int(totals[0]), "slots": int(totals[1]), "ws": self.ws_bytes, "back": int(totals[0]),
                      "enc": 8 * n, "dec": 8 * n}
        self.buf = {k: torch.full((GUARD + v + GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for k, v in self.sizes.items()}
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def close(self):
        self.L.sicn_ragged_ctx_coder_free(self.h)

    def ptr(self, name, off=0):
        return ctypes.c_void_p(self.buf[name].data_ptr() + GUARD + off)

    def inner(self, name):
        return self.buf[name][GUARD:GUARD + self.sizes[name]]

    def guards_intact(self):
        torch.cuda.synchronize()
        for name, t in self.buf.items():
            hst = t.cpu().numpy()
            assert (hst[:GUARD] == PATTERN).all() and (hst[GUARD + self.sizes[name]:] == PATTERN).all(), f"guard band of `{name}` was written"

    def untouched(self, names):
        torch.cuda.synchronize()
        for name in names:
            assert (self.buf[name].cpu().numpy() == PATTERN).all(), f"`{name}` was written"

    def encode(self, **kw):
        a = dict(h=self.h, lat=self.ptr("lat"), sc=self.ptr("scale"), out=self.ptr("slots"), status=self.ptr("enc"), ws=self.ptr("ws"),
                 ws_bytes=self.ws_bytes)
        a.update(kw)
        return self.L.sicn_ragged_ctx_encode_async(a["h"], a["lat"], a["sc"], a["out"], a["status"], a["ws"], a["ws_bytes"], self.stream)

    def decode(self, **kw):
        a = dict(h=self.h, cont=self.ptr("slots"), valid=self.ptr("enc"), sc=self.ptr("scale"), lat=self.ptr("back"), status=self.ptr("dec"),
                 ws=self.ptr("ws"), ws_bytes=self.ws_bytes)
        a.update(kw)
        return self.L.sicn_ragged_ctx_decode_async(a["h"], a["cont"], a["valid"], a["sc"], a["lat"], a["status"], a["ws"], a["ws_bytes"],
                                                   self.stream)


@pytest.mark.parametrize("lat_c", [4, 192])
def test_both_directions_stay_inside_their_buffers(codec, lat_c):
    """Latents, scales, slots, workspace, decoded latents and both status arrays, each between guard bands of 4096 bytes of 0xA5: every
    guard byte intact after the encode and after the decode.  Rotation 5 puts the uniform contents (the largest containers) first."""
    shapes = BATCHES[lat_c]
    ys, ss, wants = _case(lat_c, 5)
    call = _Call(shapes, lat_c)
    call.inner("lat").copy_(_pack(ys))
    call.inner("scale").copy_(_pack(ss))
    assert call.encode() == 0
    call.guards_intact()
    n = len(shapes)
    assert call.inner("enc").cpu().numpy().view("<i4").reshape(n, 2).tolist() == [[0, len(b)] for b in wants]
    host = call.inner("slots").cpu().numpy()
    for i, (im, b) in enumerate(zip(call.images, wants)):
        assert host[int(im.slot_offset):int(im.slot_offset) + len(b)].tobytes() == b, f"image {i}"
        tail = host[int(im.slot_offset) + len(b):int(im.slot_offset) + int(im.slot_bytes)]
        assert (tail == PATTERN).all(), f"image {i}: bytes of the slot behind its container were written"
    assert call.decode() == 0
    call.guards_intact()
    assert call.inner("dec").cpu().numpy().view("<i4").reshape(n, 2).tolist() == [[0, y.size] for y in ys]
    assert torch.equal(call.inner("back"), call.inner("lat"))
    assert np.array_equal(call.inner("slots").cpu().numpy(), host)                       # the decoder writes no slot byte
    call.close()


def test_argument_checks_return_without_launching(codec):
    """A workspace one byte short is SICN_ENOSPC, a null or misaligned pointer SICN_EINVAL, and nothing was enqueued: every output
    buffer still holds its fill pattern."""
    call = _Call(BATCHES[8], 8)
    null = ctypes.c_void_p(None)
    outputs = ["slots", "ws", "back", "enc", "dec"]
    assert call.encode(ws_bytes=call.ws_bytes - 1) == ENOSPC
    assert call.decode(ws_bytes=call.ws_bytes - 1) == ENOSPC
    assert call.encode(ws=null) == ENOSPC and call.decode(ws=null) == ENOSPC
    call.untouched(outputs)
    for kw in (dict(h=null), dict(lat=null), dict(sc=null), dict(out=null), dict(status=null), dict(lat=call.ptr("lat", 1)),
               dict(lat=call.ptr("lat", 2)), dict(sc=call.ptr("scale", 1)), dict(sc=call.ptr("scale", 2)), dict(ws=call.ptr("ws", 8))):
        assert call.encode(**kw) == EINVAL, f"encode {list(kw)}"
    for kw in (dict(h=null), dict(cont=null), dict(sc=null), dict(lat=null), dict(status=null), dict(lat=call.ptr("back", 1)),
               dict(lat=call.ptr("back", 2)), dict(sc=call.ptr("scale", 1)), dict(sc=call.ptr("scale", 2)), dict(ws=call.ptr("ws", 8)),
               dict(cont=call.ptr("slots", 1))):
        assert call.decode(**kw) == EINVAL, f"decode {list(kw)}"
    call.untouched(outputs)
    call.close()


# ---- both forms build their image from the same row: n equal shapes through the ragged coder and through the uniform entry points ----
SHARED = {"3x(37,37,192)": (3, (37, 37, 192)),     # 9 + 9 streams per image
          "3x(1,1,4)": (3, (1, 1, 4)),             # no non-anchor set: the uniform decoder launches one set only
          "2x(1,8193,4)": (2, (1, 8193, 4))}       # two anchor streams per image, the second of 4 symbols
HEADER_BYTES, TABLE_BYTES = 48, 16 * 256           # include/sicn_codec.h; csrc/k_ctx_body.hpp


@pytest.mark.parametrize("name", SHARED)
def test_ragged_and_uniform_forms_on_the_same_buffers(codec, name):
    """One latent tensor, one scale tensor, one slot buffer (slot stride = the ragged layout's) and one workspace serve a ragged
    coder of n equal shapes and sicn_codec_ctx_*_batch_async: equal containers and status words, each decoder on the other's
    containers in place, and the same verdict on an image whose valid bytes end inside its fixed part."""
    n, (h, w, c) = SHARED[name]
    rng = np.random.default_rng([n, h, w, c])
    ys, ss = zip(*[ce.CTX_CONTENTS[k]((h, w, c), rng) for k in ("uniform-uniform", "tie-up", "checkerboard")[:n]])
    call = _Call([(h, w)] * n, c)
    im, n_sym = call.images, h * w * c
    slot, ws1 = int(im[0].slot_bytes), call.ws_bytes // n
    assert [(int(x.latent_offset), int(x.slot_offset), int(x.workspace_offset), int(x.slot_bytes)) for x in im] == \
           [(i * n_sym, i * slot, i * ws1, slot) for i in range(n)]                  # a uniform batch with these three strides
    assert ws1 * n == int(call.L.sicn_codec_ctx_workspace_bytes(w, h, c, n))
    call.inner("lat").copy_(_pack(ys))
    call.inner("scale").copy_(_pack(ss))
    status = {k: torch.full((n, 2), -1, dtype=torch.int32, device="cuda") for k in ("enc_r", "enc_u", "dec_r", "dec_u")}
    sp = {k: ctypes.c_void_p(v.data_ptr()) for k, v in status.items()}

    def enc_u():
        return call.L.sicn_codec_ctx_encode_batch_async(call.ptr("lat"), call.ptr("scale"), n, w, h, c, 16 * w, 16 * h, call.ptr("slots"), slot,
                                                        sp["enc_u"], call.ptr("ws"), call.ws_bytes, call.stream)

    def dec_u(valid):
        return call.L.sicn_codec_ctx_decode_batch_async(call.ptr("slots"), slot, valid, call.ptr("scale"), n, w, h, c, call.ptr("back"),
                                                        sp["dec_u"], call.ptr("ws"), call.ws_bytes, call.stream)

    def decoded():
        torch.cuda.synchronize()
        return call.inner("back").cpu().numpy().reshape(n, n_sym)

    want = call.inner("lat").cpu().numpy().reshape(n, n_sym)
    ok = [[0, n_sym]] * n
    # the ragged encoder's containers, through the uniform decoder in place
    assert call.encode(status=sp["enc_r"]) == 0
    call.guards_intact()
    by_ragged = call.inner("slots").cpu().numpy().copy()
    call.inner("back").fill_(0xEE)
    assert dec_u(sp["enc_r"]) == 0
    assert np.array_equal(decoded(), want) and status["dec_u"].cpu().tolist() == ok
    # the uniform encoder's, on the same (refilled) slot buffer, through the ragged decoder in place
    call.inner("slots").fill_(PATTERN)
    assert enc_u() == 0
    call.guards_intact()
    assert np.array_equal(call.inner("slots").cpu().numpy(), by_ragged), "the two encoders' slot buffers differ"
    enc = status["enc_r"].cpu().tolist()
    assert enc == status["enc_u"].cpu().tolist() and [e for e, _ in enc] == [0] * n
    call.inner("back").fill_(0xEE)
    assert call.decode(valid=sp["enc_u"], status=sp["dec_r"]) == 0
    assert np.array_equal(decoded(), want) and status["dec_r"].cpu().tolist() == ok
    # image 1's valid bytes end one byte short of its fixed part (header, class tables, length table)
    fixed = HEADER_BYTES + TABLE_BYTES + 4 * (int(im[1].anchor_streams) + int(im[1].nonanchor_streams))
    assert fixed <= enc[1][1]
    valid = status["enc_u"].clone()
    valid[1, 1] = fixed - 1
    words = {}
    for key, run in (("dec_u", lambda: dec_u(ctypes.c_void_p(valid.data_ptr()))),
                     ("dec_r", lambda: call.decode(valid=ctypes.c_void_p(valid.data_ptr()), status=sp["dec_r"]))):
        status[key].fill_(-1)
        call.inner("back").fill_(0xEE)
        assert run() == 0
        got = decoded()
        words[key] = status[key].cpu().tolist()
        for i in range(n):
            if i != 1:
                assert np.array_equal(got[i], want[i]) and words[key][i] == [0, n_sym], f"{key}: image {i}"
    assert words["dec_u"] == words["dec_r"] and words["dec_u"][1][0] != 0
    call.guards_intact()
    call.close()


def test_encode_and_decode_captured_in_one_graph(codec):
    """Encode + decode captured once and replayed on fresh latents give the bytes of the eager calls."""
    shapes, lat_c = BATCHES[192], 192
    coder = codec.RaggedContextCoder(shapes, lat_c, _wh(shapes))
    eager = codec.RaggedContextCoder(shapes, lat_c, _wh(shapes))
    ys, ss, _ = _case(lat_c, 4)
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
        with torch.cuda.graph(graph, stream=side):
            enqueue()
    for rot in (5, 8):
        fy, fs, wants = _case(lat_c, rot)
        yd.copy_(_pack(fy))
        sd.copy_(_pack(fs))
        coder.slot_buffer.zero_()
        coder.enc_status.fill_(-1)
        coder.dec_status.fill_(-1)
        back.fill_(0xEE)
        graph.replay()
        eager_back = torch.full_like(yd, 0xEE)
        eager.encode(yd, sd)
        eager.decode(eager_back, sd)
        torch.cuda.synchronize()
        assert coder.containers() == eager.containers() == wants
        assert torch.equal(coder.enc_status, eager.enc_status) and torch.equal(coder.dec_status, eager.dec_status)
        assert torch.equal(back, yd) and torch.equal(eager_back, yd)


def test_ragged_hyperprior_codec_equals_the_uniform_one():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import hyperprior
    sizes, seed = [(100, 36), (64, 48), (40, 72)], 11
    rng = np.random.default_rng(211)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
    rc = hyperprior.RaggedHyperpriorCodec(sizes, seed=seed)
    z_slots, y_slots = rc.encode(rc.main.pack([torch.from_numpy(x) for x in images]))
    out = rc.decode()
    rc.check()
    containers = rc.containers()
    assert len(y_slots) == 3 and all(v.data_ptr() == s.data_ptr() for v, s in zip(y_slots, rc.y_coder.slots()))
    assert torch.equal(rc.y_hat, rc.y)
    for i, ((w, h), x) in enumerate(zip(sizes, images)):
        hc = hyperprior.HyperpriorCodec(w, h, 1, seed=seed)
        hc.encode(_dev(x[None]))
        hc.check()
        zs, ys = hc.z_coder.sizes()[0], hc.y_coder.sizes()[0]
        assert hc.z_coder.slots[0, :zs].cpu().numpy().tobytes() == containers[i][0], f"image {i}: z container"
        assert hc.y_coder.slots[0, :ys].cpu().numpy().tobytes() == containers[i][1], f"image {i}: y container"
        assert y_slots[i][:ys].cpu().numpy().tobytes() == containers[i][1]
        assert rc.bytes_per_image()[i] == zs + ys
    other = hyperprior.RaggedHyperpriorCodec(sizes, seed=seed)
    got = other.decode(z_containers=[z for z, _ in containers], y_containers=[y for _, y in containers])
    other.check()
    assert torch.equal(got, out)
