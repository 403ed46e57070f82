"""GPU checks of the ragged latent coder (include/sicn_ragged_codec.h, csrc/k_ragged_codec.hip; run with -m gpu on an MI355X): n latents
of n different shapes coded with three launches and decoded with two.  Everything is byte equality: every container against the C
oracle's (oracle/sicn_codec_oracle.c) for that image alone with the same stream length, against the uniform coder's, and every
decoded latent against what went in."""
import ctypes

import numpy as np
import pytest

from oracle import c_oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ENOSPC = -28
GUARD = 4096
PATTERN = 0xA5
LENGTHS = (1024, 2048, 8192, 16384)


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import codec as _codec
    return _codec


def _skewed(rng, shape):
    """About half zeros, a geometric tail, values < 128 — what a ReLU latent looks like to the coder."""
    n = int(np.prod(shape))
    x = np.minimum(rng.geometric(0.2, n), 127)
    x[rng.random(n) < 0.5] = 0
    return x.astype(np.uint8).reshape(shape)


def _latents(seed, shapes, lat_c):
    """One [h][w][c] latent per shape; image 1 is all zeros, image 2 one symbol value throughout, image 3 uniform over 0 .. 127."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (h, w) in enumerate(shapes):
        shape = (h, w, lat_c)
        if i == 1:
            out.append(np.zeros(shape, np.uint8))
        elif i == 2:
            out.append(np.full(shape, 37, np.uint8))
        elif i == 3:
            out.append(rng.integers(0, 128, shape, dtype=np.uint8))
        else:
            out.append(_skewed(rng, shape))
    return out


def _image_sizes(shapes):
    return [(16 * w - (i % 5), 16 * h - (i % 3)) for i, (h, w) in enumerate(shapes)]      # header fields only


def _pack(lats):
    return torch.from_numpy(np.concatenate([x.reshape(-1) for x in lats])).cuda()


def _encode(coder, lats):
    """Ragged encode of `lats`: ([container bytes], status [n][2])."""
    coder.encode(_pack(lats))
    torch.cuda.synchronize()
    st = coder.enc_status.cpu().numpy().astype(np.int64)
    host = coder.slot_buffer.cpu().numpy()
    return [host[int(im.slot_offset):int(im.slot_offset) + int(st[i, 1])].tobytes() for i, im in enumerate(coder.images[:len(lats)])], st


def _oracle(lats, sizes, lengths):
    return [c_oracle.codec_encode(x, wh, mode=3, stream_symbols=int(s)) for x, wh, s in zip(lats, sizes, lengths)]


def _assert_equals_oracle(got, st, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert st[i, 0] == 0, f"image {i}: encoder error {st[i, 0]:#x}"
        assert st[i, 1] == len(w), f"image {i}: status.bytes {st[i, 1]}, the oracle's container has {len(w)}"
        assert g == w, f"image {i}: container differs from the oracle's"


def _length_cases(n):
    return {"all-1024": [1024] * n, "all-16384": [16384] * n, "cycling": [LENGTHS[i % 4] for i in range(n)]}


def _decode(coder, n_total, slots=None, valid=None):
    back = torch.full((n_total,), 0xEE, dtype=torch.uint8, device="cuda")
    coder.decode(back, slots=slots, valid=valid)
    torch.cuda.synchronize()
    return back.cpu().numpy(), coder.dec_status.cpu().numpy().astype(np.int64)


def _assert_round_trip(back, st, lats):
    off = 0
    for i, x in enumerate(lats):
        assert st[i, 0] == 0, f"image {i}: decoder error {st[i, 0]:#x}"
        assert st[i, 1] == x.size
        assert np.array_equal(back[off:off + x.size], x.reshape(-1)), f"image {i}: decoded latent differs"
        off += x.size


# ---- 1 .. 3: bytes against the oracle ------------------------------------------------------------------------------------------
EDGE_N = [1, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 - 5, 16384, 16385]


@pytest.mark.parametrize("case", ["all-1024", "all-16384", "cycling"])
def test_stream_cut_edges_equal_the_oracle(codec, case):
    shapes = [(1, n) for n in EDGE_N]
    lengths = _length_cases(len(shapes))[case]
    lats, sizes = _latents(11, shapes, 1), _image_sizes(shapes)
    coder = codec.RaggedLatentCoder(shapes, 1, sizes, lengths)
    got, st = _encode(coder, lats)
    _assert_equals_oracle(got, st, _oracle(lats, sizes, lengths))
    _assert_round_trip(*_decode(coder, sum(EDGE_N)), lats)


@pytest.mark.parametrize("case", ["all-1024", "all-16384", "cycling"])
def test_unaligned_image_starts_equal_the_oracle(codec, case):
    shapes = [(7, 3), (1, 1), (11, 13), (9, 2), (3, 5), (1, 2), (21, 17)]                  # lat_c = 5: offsets 105, 110, 825, ..
    lengths = _length_cases(len(shapes))[case]
    lats, sizes = _latents(12, shapes, 5), _image_sizes(shapes)
    coder = codec.RaggedLatentCoder(shapes, 5, sizes, lengths)
    assert any(int(im.latent_offset) % 4 for im in coder.images) and any(int(im.latent_offset) % 16 for im in coder.images)
    got, st = _encode(coder, lats)
    _assert_equals_oracle(got, st, _oracle(lats, sizes, lengths))
    _assert_round_trip(*_decode(coder, sum(x.size for x in lats)), lats)


NET_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 3), (3, 3), (3, 5), (2, 7), (3, 7), (12, 16)]    # (lat_h, lat_w), 192 channels


@pytest.mark.parametrize("case", ["all-1024", "all-16384", "cycling"])
def test_net_latents_equal_the_oracle_and_the_uniform_coder(codec, case):
    lengths = _length_cases(len(NET_SHAPES))[case]
    lats, sizes = _latents(13, NET_SHAPES, 192), _image_sizes(NET_SHAPES)
    coder = codec.RaggedLatentCoder(NET_SHAPES, 192, sizes, lengths)
    got, st = _encode(coder, lats)
    _assert_equals_oracle(got, st, _oracle(lats, sizes, lengths))
    for i, (x, (w, h), s) in enumerate(zip(lats, sizes, lengths)):
        # the asynchronous uniform coder on this image alone, with the same stream length ...
        one = codec.LatentCoder(1, x.shape[0], x.shape[1], 192, w, h, stream_symbols=s)
        one.encode(torch.from_numpy(x[None]).cuda())
        torch.cuda.synchronize()
        assert one.slots[0, :one.sizes()[0]].cpu().numpy().tobytes() == got[i], f"image {i}: differs from LatentCoder alone"
        if s == 16384:   # ... and codec.encode_latent, which writes the format's default length
            alone = codec.encode_latent(torch.from_numpy(x).cuda(), w, h)
            assert alone.cpu().numpy().tobytes() == got[i], f"image {i}: differs from encode_latent alone"


def test_default_stream_length_is_each_images_own(codec):
    shapes = [(2, 3), (120, 120)]                                   # 1152 and 2.76 M symbols: 8192 and 16384
    coder = codec.RaggedLatentCoder(shapes, 192)
    assert coder.stream_symbols == [codec.auto_stream_symbols(2 * 3 * 192), codec.auto_stream_symbols(120 * 120 * 192)] == [8192, 16384]


# ---- 4: round trip and cross-decoding ---------------------------------------------------------------------------------------
def test_round_trip_and_cross_decoding(codec):
    lengths = _length_cases(len(NET_SHAPES))["cycling"]
    lats, sizes = _latents(14, NET_SHAPES, 192), _image_sizes(NET_SHAPES)
    total = sum(x.size for x in lats)
    coder = codec.RaggedLatentCoder(NET_SHAPES, 192, sizes, lengths)
    got, _ = _encode(coder, lats)
    _assert_round_trip(*_decode(coder, total), lats)
    # containers the ORACLE made, copied into slots of our own, their lengths as the valid bytes
    want = _oracle(lats, sizes, lengths)
    host = np.full(coder.slot_bytes, PATTERN, np.uint8)
    for c, im in zip(want, coder.images):
        host[int(im.slot_offset):int(im.slot_offset) + len(c)] = np.frombuffer(c, np.uint8)
    valid = torch.tensor([[0, len(c)] for c in want], dtype=torch.int32, device="cuda")
    _assert_round_trip(*_decode(coder, total, slots=torch.from_numpy(host).cuda(), valid=valid), lats)
    # the same through for_containers, which reads shapes and stream lengths from the headers
    other = codec.RaggedLatentCoder.for_containers(want)
    assert other.shapes == NET_SHAPES and other.stream_symbols == lengths and other.image_sizes == sizes
    _assert_round_trip(*_decode(other, total), lats)
    # every ragged container through the single-image decoder
    for i, (c, x) in enumerate(zip(got, lats)):
        back, info = codec.decode_latent(torch.from_numpy(np.frombuffer(c, np.uint8).copy()).cuda())
        assert np.array_equal(back.cpu().numpy(), x), f"image {i}: decode_latent of the ragged container differs"
        assert int(info.stream_symbols) == lengths[i]


# ---- 5: the two-table decode form ---------------------------------------------------------------------------------------------
def test_two_table_decode_form(codec):
    shapes = [(1, 5), (1, 1400 * 1024 - 3), (2, 2), (1, 1025)]      # 1400 streams + 4: more than 5 x 256 in all
    lengths = [1024] * 4
    lats, sizes = _latents(15, shapes, 1), _image_sizes(shapes)
    lats[1] = _skewed(np.random.default_rng(151), lats[1].shape)    # the large one carries real statistics
    coder = codec.RaggedLatentCoder(shapes, 1, sizes, lengths)
    assert sum(int(im.n_streams) for im in coder.images[:4]) == 1400 + 1 + 1 + 2 > 5 * 256
    got, st = _encode(coder, lats)
    _assert_equals_oracle(got, st, _oracle(lats, sizes, lengths))
    _assert_round_trip(*_decode(coder, sum(x.size for x in lats)), lats)


# ---- 6: a deep table ----------------------------------------------------------------------------------------------------------
def test_seventy_tiny_images(codec):
    shapes = [(1 + i % 3, 1 + (i // 3) % 3) for i in range(70)]
    lats, sizes = _latents(16, shapes, 192), _image_sizes(shapes)
    coder = codec.RaggedLatentCoder(shapes, 192, sizes)
    got, st = _encode(coder, lats)
    _assert_equals_oracle(got, st, _oracle(lats, sizes, coder.stream_symbols))
    _assert_round_trip(*_decode(coder, sum(x.size for x in lats)), lats)
    assert coder.containers() == got and coder.sizes() == [len(c) for c in got]


# ---- 7: order -------------------------------------------------------------------------------------------------------------------
def test_permuting_the_batch_permutes_the_containers(codec):
    lengths = _length_cases(len(NET_SHAPES))["cycling"]
    lats, sizes = _latents(17, NET_SHAPES, 192), _image_sizes(NET_SHAPES)
    got, _ = _encode(codec.RaggedLatentCoder(NET_SHAPES, 192, sizes, lengths), lats)
    perm = [4, 8, 0, 6, 2, 7, 1, 5, 3]
    pick = lambda seq: [seq[p] for p in perm]
    got_p, st_p = _encode(codec.RaggedLatentCoder(pick(NET_SHAPES), 192, pick(sizes), pick(lengths)), pick(lats))
    assert not st_p[:, 0].any()
    assert got_p == pick(got)


# ---- 8: errors stay with their image ----------------------------------------------------------------------------------------
def test_encode_error_stays_with_its_image(codec):
    lats, sizes = _latents(18, NET_SHAPES, 192), _image_sizes(NET_SHAPES)
    coder = codec.RaggedLatentCoder(NET_SHAPES, 192, sizes, 2048)
    clean, _ = _encode(coder, lats)
    bad = [x.copy() for x in lats]
    bad[5].reshape(-1)[77] = 200                                    # a symbol >= 128 in image 5
    got, st = _encode(coder, bad)
    assert st[5, 0] & 1
    for i in range(len(lats)):
        if i != 5:
            assert st[i, 0] == 0 and got[i] == clean[i], f"image {i} changed beside a bad one"


def test_decode_errors_stay_with_their_image(codec):
    lats, sizes = _latents(19, NET_SHAPES, 192), _image_sizes(NET_SHAPES)
    total = sum(x.size for x in lats)
    coder = codec.RaggedLatentCoder(NET_SHAPES, 192, sizes, 2048)
    _encode(coder, lats)
    enc = coder.enc_status.clone()

    def others_exact(back, st, victim):
        off = 0
        for i, x in enumerate(lats):
            if i != victim:
                assert st[i, 0] == 0 and st[i, 1] == x.size, f"image {i}: status {st[i]} beside a bad container"
                assert np.array_equal(back[off:off + x.size], x.reshape(-1)), f"image {i}: latent differs beside a bad container"
            off += x.size

    # a payload byte flipped in slot 8 (18 streams): malformed (bits 2-6) or checksum (bit 7), nothing else touched
    im = coder.images[8]
    fixed = 48 + 256 + 4 * int(im.n_streams)
    slots = coder.slot_buffer.clone()
    slots[int(im.slot_offset) + fixed + (int(enc[8, 1]) - fixed) // 2] ^= 0x5A
    back, st = _decode(coder, total, slots=slots, valid=enc)
    assert st[8, 0] & 0xFC and not st[8, 0] & ~0xFC, f"{st[8, 0]:#x}"
    others_exact(back, st, 8)
    # `valid` of image 4 one byte shorter than its fixed part: bit 8, the slot is not read
    short = enc.clone()
    short[4, 1] = 48 + 256 + 4 * int(coder.images[4].n_streams) - 1
    back, st = _decode(coder, total, valid=short)
    assert st[4, 0] & 0x100
    others_exact(back, st, 4)
    # and the undamaged slots still decode
    _assert_round_trip(*_decode(coder, total), lats)


# ---- 9: stays inside its buffers ----------------------------------------------------------------------------------------------
def test_stays_inside_its_buffers(codec):
    from simple_image_compression_network_amd import _lib
    L = _lib.lib()
    shapes = [(7, 3), (1, 1), (11, 13), (9, 2), (40, 30)]
    lengths = [1024, 2048, 8192, 16384, 1024]
    lats, sizes = _latents(20, shapes, 5), _image_sizes(shapes)
    coder = codec.RaggedLatentCoder(shapes, 5, sizes, lengths)
    n = len(shapes)
    ws_bytes = int(L.sicn_ragged_coder_workspace_bytes(coder._h))
    guarded = lambda nbytes: torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    slots, ws, back = guarded(coder.slot_bytes), guarded(ws_bytes), guarded(coder.latent_bytes)
    packed = _pack(lats)
    enc = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    dec = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def untouched(t, nbytes):
        h = t.cpu().numpy()
        return (h[:GUARD] == PATTERN).all() and (h[GUARD + nbytes:] == PATTERN).all()

    # a workspace one byte short: SICN_ENOSPC and nothing enqueued
    assert L.sicn_ragged_coder_encode_async(coder._h, ptr(packed), ptr(slots, GUARD), ptr(enc), ptr(ws, GUARD), ws_bytes - 1, stream) == ENOSPC
    assert L.sicn_ragged_coder_decode_async(coder._h, ptr(slots, GUARD), None, ptr(back, GUARD), ptr(dec), ptr(ws, GUARD), ws_bytes - 1, stream) == ENOSPC
    torch.cuda.synchronize()
    for t in (slots, ws, back):
        assert (t.cpu().numpy() == PATTERN).all()
    assert not enc.any() and not dec.any()

    assert L.sicn_ragged_coder_encode_async(coder._h, ptr(packed), ptr(slots, GUARD), ptr(enc), ptr(ws, GUARD), ws_bytes, stream) == 0
    assert L.sicn_ragged_coder_decode_async(coder._h, ptr(slots, GUARD), ptr(enc), ptr(back, GUARD), ptr(dec), ptr(ws, GUARD), ws_bytes, stream) == 0
    torch.cuda.synchronize()
    assert untouched(slots, coder.slot_bytes) and untouched(ws, ws_bytes) and untouched(back, coder.latent_bytes)
    st, host = enc.cpu().numpy().astype(np.int64), slots.cpu().numpy()[GUARD:GUARD + coder.slot_bytes]
    want = _oracle(lats, sizes, lengths)
    for i, im in enumerate(coder.images[:n]):
        a, size, cap = int(im.slot_offset), int(st[i, 1]), int(im.slot_bytes)
        assert st[i, 0] == 0 and host[a:a + size].tobytes() == want[i]
        assert size < cap and (host[a + size:a + cap] == PATTERN).all(), f"slot {i}: bytes behind the container were written"
    _assert_round_trip(back.cpu().numpy()[GUARD:GUARD + coder.latent_bytes], dec.cpu().numpy().astype(np.int64), lats)


# ---- 10: capture ----------------------------------------------------------------------------------------------------------------
def test_encode_and_decode_are_graph_capturable(codec):
    lengths = _length_cases(len(NET_SHAPES))["cycling"]
    sizes = _image_sizes(NET_SHAPES)
    first, fresh = _latents(21, NET_SHAPES, 192), _latents(22, NET_SHAPES, 192)
    coder = codec.RaggedLatentCoder(NET_SHAPES, 192, sizes, lengths)
    want, want_st = _encode(coder, fresh)                           # eager, on the latents the replay will see (also the warm-up)
    _assert_round_trip(*_decode(coder, coder.latent_bytes), fresh)
    x = _pack(first)
    back = torch.zeros(coder.latent_bytes, dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            coder.encode(x)
            coder.decode(back, valid=coder.enc_status)
    x.copy_(_pack(fresh))
    coder.slot_buffer.zero_()
    coder.enc_status.zero_()
    coder.dec_status.fill_(-1)
    back.zero_()
    graph.replay()
    torch.cuda.synchronize()
    st = coder.enc_status.cpu().numpy().astype(np.int64)
    host = coder.slot_buffer.cpu().numpy()
    got = [host[int(im.slot_offset):int(im.slot_offset) + int(st[i, 1])].tobytes() for i, im in enumerate(coder.images[:len(fresh)])]
    assert np.array_equal(st, want_st) and got == want
    _assert_round_trip(back.cpu().numpy(), coder.dec_status.cpu().numpy().astype(np.int64), fresh)


# ---- 11: end to end with RaggedNet ------------------------------------------------------------------------------------------
def test_ragged_net_compress_and_decompress(codec):
    from simple_image_compression_network_amd import api
    from simple_image_compression_network_amd.config import eight_layer_descs
    sizes = [(17, 9), (33, 20), (48, 48), (100, 36), (64, 17), (21, 35), (90, 10), (77, 31)]      # (width, height)
    weights = [api.DeviceWeights(d, w, b) for d, (w, b) in zip(eight_layer_descs(16, 16), api.load_param_weights())]
    rng = np.random.default_rng(23)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
    net = api.RaggedNet(sizes, shared_weights=weights)
    xin = net.pack([torch.from_numpy(x) for x in images])
    containers = net.compress(xin)
    assert len(containers) == len(sizes)
    for i, ((w, h), x) in enumerate(zip(sizes, images)):
        one = api.EightLayersNet(descs=eight_layer_descs(w, h), shared_weights=weights)
        _, lat = one.forward(torch.from_numpy(x[None]).cuda())
        alone = codec.encode_latent(lat[0].contiguous(), w, h)
        torch.cuda.synchronize()
        assert alone.cpu().numpy().tobytes() == containers[i], f"image {i}: container differs from EightLayersNet + encode_latent"
    want, _ = net.forward(xin)
    got = net.decompress(containers)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # the coder the net hands out: its boundary-3 shapes, its image sizes, each image's own stream length
    coder = net.latent_coder()
    assert [(h, w, coder.lat_c) for h, w in coder.shapes] == net.shapes(3) and coder.image_sizes == sizes
    assert coder.stream_symbols == [codec.auto_stream_symbols(h * w * c) for h, w, c in net.shapes(3)]
