"""GPU checks of the uniform coders' bookkeeping kernels through the C entry points: the scan form of mode 3 (more than 2048 streams per
image, or none) and mode 4, every image of a batch, on buffers that lie between guard bands inside larger tensors.  Containers are
compared with oracle.c_oracle byte for byte, never with this library's own output."""
import ctypes
import functools

import numpy as np
import pytest

import codec_edge_cases as ce
from oracle import c_oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 4096
PATTERN = 0xA5
HEADER = ce.HEADER


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import _lib
    return _lib.lib()


class _Buffers:
    """Named byte buffers, each a view behind and in front of GUARD bytes of PATTERN inside its own larger tensor."""

    def __init__(self, **sizes):
        self.sizes = sizes
        self.buf = {k: torch.full((GUARD + v + GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ptr(self, name, off=0):
        return ctypes.c_void_p(self.buf[name].data_ptr() + GUARD + off)

    def inner(self, name):
        return self.buf[name][GUARD:GUARD + self.sizes[name]]

    def status(self, name):
        torch.cuda.synchronize()
        return self.inner(name).cpu().numpy().view("<u4").reshape(-1, 2).tolist()

    def guards_intact(self):
        torch.cuda.synchronize()
        for name, t in self.buf.items():
            end = GUARD + self.sizes[name]
            assert bool((t[:GUARD] == PATTERN).all()) and bool((t[end:] == PATTERN).all()), f"guard band of `{name}` was written"


# ---- mode 3, scan form ------------------------------------------------------------------------------------------------------------
WSS3 = 1024
CAP3 = 2 * WSS3 + 256                        # scratch / largest stream of 1024 symbols (wstream_cap, csrc/k_codec_body.hpp)
SCAN_SHAPE = (1, 2049 * 1024 + 5, 1)         # 2050 streams, the last of 5 symbols: the smallest latent above SELF_SCAN_MAX = 2048
SCAN_IMAGES = 3


@functools.lru_cache(maxsize=None)
def _scan_case():
    """([latent], [oracle container]) of the scan-form batch: skewed symbols below 128, another seed per image; computed once, read-only."""
    ys = [np.minimum(np.random.default_rng([3, i]).geometric(0.2 + 0.1 * i, SCAN_SHAPE) - 1, 127).astype(np.uint8) for i in range(SCAN_IMAGES)]
    for y in ys:
        y.setflags(write=False)
    return ys, [c_oracle.codec_encode(y, (16 * SCAN_SHAPE[1], 16), mode=3, stream_symbols=WSS3) for y in ys]


def test_scan_form_every_image_inside_its_buffers(L):
    """Three images of 2050 streams through sicn_codec_{encode,decode}_batch_async_sl at 1024 symbols per stream, workspace of exactly
    sicn_codec_batch_workspace_bytes_sl: oracle bytes and exact status pairs per image, the round trip, every guard byte of latents,
    slots, workspace, decoded latents and both status arrays intact after each direction.  Then two damaged inputs, each isolated to
    its image.  A length-table entry above the cap (2304) counts as 0 in the scan: image 1 reports exactly 0x60, bit 5 for the entry
    and the streams behind it, bit 6 because the table no longer adds up to the payload field.  Valid bytes that end inside image
    2's fixed part: the parse stage says 0x104 and gives the streams a payload of 0 bytes, the scan skips the table, every stream
    fails its bound and raises the stream-error word, so the finish stage reports exactly 0x124 (0x104 and bit 5, the word the
    self form documents for the same input; a bare 0x104 is what the parse stage alone says), and no byte of the latent is written.
    Both words are what the previous library reports too."""
    h, w, c = SCAN_SHAPE
    n, k = h * w * c, SCAN_IMAGES
    ns = (n + WSS3 - 1) // WSS3
    assert ns == 2050
    ys, wants = _scan_case()
    slot = int(L.sicn_codec_max_bytes_sl(n, WSS3))
    ws_bytes = int(L.sicn_codec_batch_workspace_bytes_sl(n, k, WSS3))
    assert slot % 2 == 0 and all(len(b) <= slot for b in wants)
    b = _Buffers(lat=k * n, slots=k * slot, ws=ws_bytes, back=k * n, enc=8 * k, dec=8 * k)
    b.inner("lat").copy_(torch.from_numpy(np.concatenate([y.reshape(-1) for y in ys])).cuda())

    def decode(valid):
        b.inner("back").fill_(0xEE)
        b.inner("dec").fill_(0xFF)
        assert L.sicn_codec_decode_batch_async_sl(b.ptr("slots"), slot, valid, k, w, h, c, b.ptr("back"), n, b.ptr("dec"), b.ptr("ws"),
                                                  ws_bytes, b.stream, WSS3) == 0
        b.guards_intact()
        return b.status("dec"), b.inner("back").cpu().numpy().reshape(k, n)

    assert L.sicn_codec_encode_batch_async_sl(b.ptr("lat"), k, w, h, c, 16 * w, 16 * h, b.ptr("slots"), slot, b.ptr("enc"), b.ptr("ws"),
                                              ws_bytes, b.stream, WSS3) == 0
    b.guards_intact()
    assert b.status("enc") == [[0, len(x)] for x in wants]
    good = b.inner("slots").clone()
    host = good.cpu().numpy()
    for i, x in enumerate(wants):
        assert host[i * slot:i * slot + len(x)].tobytes() == x, f"image {i}"
    status, back = decode(b.ptr("enc"))
    assert status == [[0, n]] * k
    for i, y in enumerate(ys):
        assert np.array_equal(back[i], y.reshape(-1)), f"image {i}"
    assert torch.equal(b.inner("slots"), good)                           # the decoder writes no slot byte

    entry = slot + HEADER + 256 + 4 * 1000                               # stream 1000 of image 1
    b.inner("slots")[entry:entry + 4].copy_(torch.from_numpy(np.frombuffer(int(CAP3 + 2).to_bytes(4, "little"), np.uint8).copy()).cuda())
    status, back = decode(b.ptr("enc"))
    assert status[0] == [0, n] and status[2] == [0, n]
    assert status[1] == [0x60, n]
    for i in (0, 2):
        assert np.array_equal(back[i], ys[i].reshape(-1)), f"image {i}"

    b.inner("slots").copy_(good)
    valid = torch.from_numpy(np.array([[0, len(x)] for x in wants], "<u4")).cuda()
    valid[2, 1] = HEADER + 256 + 4 * ns - 1
    status, back = decode(ctypes.c_void_p(valid.data_ptr()))
    assert status == [[0, n], [0, n], [0x124, n]]
    assert (back[2] == 0xEE).all(), "a byte of the rejected image's latent was written"
    for i in (0, 1):
        assert np.array_equal(back[i], ys[i].reshape(-1)), f"image {i}"


def test_empty_latents_in_a_batch(L):
    """Two images of shape (0, 4, 4): the encoder's scan branch without a stream, at blockIdx.y = 1 too.  Both containers are the
    oracle's 304 bytes (header and an all-zero frequency table), both status pairs exact, all guard bytes intact."""
    want = c_oracle.codec_encode(np.zeros((0, 4, 4), np.uint8), (64, 48), mode=3)
    assert len(want) == HEADER + 256 == 304
    slot = int(L.sicn_codec_max_bytes_sl(0, ce.WSS))
    ws_bytes = int(L.sicn_codec_batch_workspace_bytes_sl(0, 2, ce.WSS))
    assert slot == 304
    b = _Buffers(lat=16, slots=2 * slot, ws=ws_bytes, enc=16)
    assert L.sicn_codec_encode_batch_async_sl(b.ptr("lat"), 2, 4, 0, 4, 64, 48, b.ptr("slots"), slot, b.ptr("enc"), b.ptr("ws"), ws_bytes,
                                              b.stream, ce.WSS) == 0
    b.guards_intact()
    assert b.status("enc") == [[0, 304], [0, 304]]
    host = b.inner("slots").cpu().numpy()
    assert host[:304].tobytes() == want and host[304:].tobytes() == want
    assert bool((b.inner("lat") == PATTERN).all())


# ---- mode 4 -----------------------------------------------------------------------------------------------------------------------
CTX_SHAPES = {"3x(9,10,192)": (9, 10, 192),      # one anchor and one non-anchor stream
              "3x(1,1,4)": (1, 1, 4)}            # no non-anchor stream: the decoder launches one set only


@pytest.mark.parametrize("name", CTX_SHAPES)
def test_uniform_context_coder_inside_its_buffers(L, name):
    """Three images through sicn_codec_ctx_{encode,decode}_batch_async, workspace of exactly sicn_codec_ctx_workspace_bytes: oracle
    bytes and exact status words per image, the round trip, every guard byte intact after each direction."""
    h, w, c = CTX_SHAPES[name]
    n, k = h * w * c, 3
    assert ce.ctx_geometry(h, w, c)[1] == ((1, 1) if n > 4 else (1, 0))
    rng = np.random.default_rng([4, h, w, c])
    ys, ss = zip(*[ce.CTX_CONTENTS[key]((h, w, c), rng) for key in ("uniform-uniform", "checkerboard", "uniform-s0")])
    wants = [c_oracle.ctx_encode(y, s, (16 * w, 16 * h)) for y, s in zip(ys, ss)]
    slot = (int(L.sicn_codec_ctx_max_bytes(w, h, c)) + 1) & ~1
    ws_bytes = int(L.sicn_codec_ctx_workspace_bytes(w, h, c, k))
    b = _Buffers(lat=k * n, scale=k * n, slots=k * slot, ws=ws_bytes, back=k * n, enc=8 * k, dec=8 * k)
    b.inner("lat").copy_(torch.from_numpy(np.concatenate([y.reshape(-1) for y in ys])).cuda())
    b.inner("scale").copy_(torch.from_numpy(np.concatenate([s.reshape(-1) for s in ss])).cuda())
    assert L.sicn_codec_ctx_encode_batch_async(b.ptr("lat"), b.ptr("scale"), k, w, h, c, 16 * w, 16 * h, b.ptr("slots"), slot, b.ptr("enc"),
                                               b.ptr("ws"), ws_bytes, b.stream) == 0
    b.guards_intact()
    assert b.status("enc") == [[0, len(x)] for x in wants]
    host = b.inner("slots").cpu().numpy()
    for i, x in enumerate(wants):
        assert host[i * slot:i * slot + len(x)].tobytes() == x, f"image {i}"
        assert (host[i * slot + len(x):(i + 1) * slot] == PATTERN).all(), f"image {i}: bytes of the slot behind its container were written"
    b.inner("back").fill_(0xEE)
    assert L.sicn_codec_ctx_decode_batch_async(b.ptr("slots"), slot, b.ptr("enc"), b.ptr("scale"), k, w, h, c, b.ptr("back"), b.ptr("dec"),
                                               b.ptr("ws"), ws_bytes, b.stream) == 0
    b.guards_intact()
    assert b.status("dec") == [[0, n]] * k
    assert torch.equal(b.inner("back"), b.inner("lat"))
    assert np.array_equal(b.inner("slots").cpu().numpy(), host)          # the decoder writes no slot byte
