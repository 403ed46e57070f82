"""Latent container + rANS coder.  NEW functionality without a reference
counterpart, parity "unpinned": the CPU tests pin the oracle's own specification (round trips, header,
frequency normalisation, corruption detection); the GPU tests show GPU == oracle byte for byte and
decode(encode(x)) == x on the real latent of the net."""
import ctypes
import re
import struct
import zlib
from pathlib import Path

import numpy as np
import pytest

from oracle import c_oracle

ROOT = Path(__file__).resolve().parent.parent


def _mock_latent(rng, shape, zero_frac=0.5):
    """Like the net's latent: ~50 % zeros, the rest uniform on 1..127."""
    lat = rng.integers(1, 128, shape, dtype=np.uint8)
    lat[rng.random(shape) < zero_frac] = 0
    return lat


SHAPES = [(16, 16, 192), (1, 1, 192), (3, 5, 7), (0, 4, 4), (2, 2, 1), (8, 3, 192), (64, 1, 16), (1, 1, 64), (1, 1, 65),
          (9, 10, 192)]   # the last one: 17280 symbols = one full 16384-symbol wave stream + a short one


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_oracle_round_trip(shape, mode):
    rng = np.random.default_rng(sum(shape) * 3 + mode)
    lat = _mock_latent(rng, shape)
    blob = c_oracle.codec_encode(lat, (shape[1] * 16, shape[0] * 16), mode)
    out, info = c_oracle.codec_decode(blob)
    assert np.array_equal(out, lat)
    assert info.tolist()[:6] == [mode, shape[1] * 16, shape[0] * 16, shape[1], shape[0], shape[2]]
    assert len(blob) <= c_oracle.lib().sicl_or_max_bytes(mode, lat.size)


def test_header_fields_and_checksum():
    lat = _mock_latent(np.random.default_rng(1), (4, 6, 8))
    blob = c_oracle.codec_encode(lat, (96, 64), 2)
    magic, ver, mode, iw, ih, lw, lh, lc, n, ns, ss, payload, adler = struct.unpack("<4sHHIIIIIIIIII", blob[:48])
    assert (magic, ver, mode, iw, ih, lw, lh, lc, n, ns, ss) == (b"SICL", 1, 2, 96, 64, 6, 4, 8, 192, 1, 1024)
    assert adler == zlib.adler32(lat.tobytes())            # the header checksum is the standard adler32
    freq = np.frombuffer(blob[48:48 + 256], "<u2")
    assert int(freq.sum()) == 4096 and all(freq[s] > 0 for s in np.unique(lat))
    (len0,) = struct.unpack("<I", blob[304:308])
    assert payload == len0 == len(blob) - 308


def test_extreme_distributions_round_trip():
    rng = np.random.default_rng(2)
    for lat in (np.zeros((4, 4, 192), np.uint8), np.full((4, 4, 192), 127, np.uint8),
                np.arange(128, dtype=np.uint8).reshape(1, 1, 128),
                np.concatenate([np.zeros(5000, np.uint8), np.array([77], np.uint8)]).reshape(1, 1, -1),   # freq 1 symbol
                rng.integers(0, 128, (5, 41, 6), dtype=np.uint8)):
        for mode in (0, 1, 2, 3):
            out, _ = c_oracle.codec_decode(c_oracle.codec_encode(lat, (0, 0), mode))
            assert np.array_equal(out, lat)
    # a constant latent costs almost nothing under rANS: 4 state bytes + <= 1 byte per 1024-symbol stream
    blob = c_oracle.codec_encode(np.zeros((16, 16, 192), np.uint8), (256, 256), 2)
    assert len(blob) < 48 + 256 + 48 * 4 + 48 * 8


def test_wave_form_layout():
    """Mode 3: stream_symbols 16384, per stream 64 little-endian u32 states then 16-bit words; one state per lane
    even for a stream shorter than 64 symbols, and the idle lanes keep the initial state 2^16."""
    lat = _mock_latent(np.random.default_rng(8), (1, 1, 40))
    blob = c_oracle.codec_encode(lat, (16, 16), 3)
    magic, ver, mode, iw, ih, lw, lh, lc, n, ns, ss, payload, adler = struct.unpack("<4sHHIIIIIIIIII", blob[:48])
    assert (mode, n, ns, ss) == (3, 40, 1, 16384)
    (len0,) = struct.unpack("<I", blob[304:308])
    assert payload == len0 == len(blob) - 308 and len0 % 2 == 0 and len0 >= 256
    states = np.frombuffer(blob[308:308 + 256], "<u4")   # 40 symbols = 4 per lane on lanes 0..9
    assert np.all(states[10:] == 1 << 16) and np.all(states[:10] >= 1 << 16)
    # the wave form costs at most the 252 extra flush bytes per stream plus word granularity
    big = _mock_latent(np.random.default_rng(9), (32, 32, 192))
    a, b = len(c_oracle.codec_encode(big, (0, 0), 2)), len(c_oracle.codec_encode(big, (0, 0), 3))
    assert b < a * 1.02


@pytest.mark.parametrize("ss", [1024, 2048, 4096, 8192, 16384])
def test_stream_length_is_an_encoder_parameter(ss):
    """Mode 3 with the encoder's choice of stream length (header dword 9): round trip, stream count, the default entry point
    = 16384, inadmissible lengths rejected; shorter streams cost 260 bytes each (64 final states + the length entry)."""
    shape = (9, 10, 192)                                   # 17280 symbols: ragged last stream at every length
    lat = _mock_latent(np.random.default_rng(21), shape)
    blob = c_oracle.codec_encode(lat, (160, 144), 3, stream_symbols=ss)
    magic, ver, mode, iw, ih, lw, lh, lc, n, ns, hss, payload, adler = struct.unpack("<4sHHIIIIIIIIII", blob[:48])
    assert (mode, n, ns, hss) == (3, 17280, -(-17280 // ss), ss)
    out, _ = c_oracle.codec_decode(blob)
    assert np.array_equal(out, lat)
    assert len(blob) <= c_oracle.lib().sicl_or_max_bytes_sl(3, lat.size, ss)
    ref = c_oracle.codec_encode(lat, (160, 144), 3)
    if ss == 16384:
        assert blob == ref
    else:   # every extra stream costs its 64 final states + length entry, give or take the words the states absorb
        extra = ns - 2
        assert 0 < len(blob) - len(ref) <= 260 * extra + 64
    lens = np.frombuffer(blob[304:304 + 4 * ns], "<u4")
    assert int(lens.sum()) == payload and np.all(lens >= 256) and np.all(lens % 2 == 0)
    for bad in (0, 512, 3000, 32768):
        with pytest.raises(RuntimeError):
            c_oracle.codec_encode(lat, (0, 0), 3, stream_symbols=bad)
    with pytest.raises(RuntimeError):
        c_oracle.codec_encode(lat, (0, 0), 2, stream_symbols=4096)      # mode 2 has one stream length
    hostile = bytearray(blob)
    hostile[36:40] = struct.pack("<I", 3000)                             # a header naming a length the format does not have
    with pytest.raises(RuntimeError):
        c_oracle.codec_decode(bytes(hostile))


def test_auto_stream_length_policy():
    """codec.auto_stream_symbols: a function of ONE image's latent (never of the batch: a container set written by a batch of 8
    must decode in a batch of 1) — the format's 16384 for latents of >= 128 such streams, 8192 (+ 2.8 % bytes, half
    the serial chain) below."""
    from simple_image_compression_network_amd import codec
    n4k, n1080, nz = 135 * 240 * 192, 68 * 120 * 192, 34 * 60 * 128
    for k in (1, 3, 8):
        assert codec.auto_stream_symbols(n4k, k) == 16384          # 380 streams per image
        assert codec.auto_stream_symbols(n1080, k) == 8192         # 192 streams
        assert codec.auto_stream_symbols(nz, k) == 8192            # the hyperprior's hyper-latent of a 4K image
        assert codec.auto_stream_symbols(1000, k) == 8192 and codec.auto_stream_symbols(0, k) == 8192
    assert codec.auto_stream_symbols(128 * 16384) == 16384 and codec.auto_stream_symbols(128 * 16384 - 1) == 8192


def test_rejects_symbols_over_127_and_corruption():
    lat = _mock_latent(np.random.default_rng(3), (4, 4, 192))
    bad = lat.copy()
    bad[0, 0, 0] = 200
    with pytest.raises(RuntimeError):
        c_oracle.codec_encode(bad, (0, 0), 2)
    for mode in (2, 3):
        blob = bytearray(c_oracle.codec_encode(lat, (64, 64), mode))
        blob[-5] ^= 0x40                                   # flip a payload bit
        with pytest.raises(RuntimeError):
            c_oracle.codec_decode(bytes(blob))
    with pytest.raises(RuntimeError):
        c_oracle.codec_decode(bytes(blob[:40]))            # truncated header


def test_frequency_normalisation_properties():
    L = c_oracle.lib()
    rng = np.random.default_rng(4)
    for _ in range(50):
        k = int(rng.integers(1, 129))
        h = np.zeros(128, np.uint32)
        h[rng.choice(128, k, replace=False)] = rng.integers(1, 1 << int(rng.integers(1, 24)), k)
        f = np.zeros(128, np.uint16)
        assert L.sicl_or_normalize(c_oracle._ptr(h), int(h.sum()), c_oracle._ptr(f)) == 0
        assert int(f.sum()) == 4096 and np.array_equal(f > 0, h > 0)


def test_codec_abi_symbols_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sicn_codec.h").read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(sicn_codec_[a-z0-9_]+)\s*\(", text)))
    from simple_image_compression_network_amd import _lib
    L = _lib.lib()        # (loads the HIP runtime PyTorch ships first, then libsicn.so)
    assert set(syms) == set(_lib.CODEC_ABI) and all(hasattr(L, s) for s in syms)
    info = _lib.CodecInfo()
    blob = c_oracle.codec_encode(_mock_latent(np.random.default_rng(5), (2, 3, 4)), (48, 32), 1)
    buf = (ctypes.c_uint8 * 48).from_buffer_copy(blob[:48])
    assert _lib.lib().sicn_codec_parse_header(buf, 48, ctypes.byref(info)) == 0        # pure host function
    assert (info.mode, info.image_width, info.lat_w, info.lat_h, info.lat_c, info.n_symbols) == (1, 48, 3, 2, 4, 24)
    assert _lib.lib().sicn_codec_parse_header(buf, 10, ctypes.byref(info)) == -22


def test_ransw_div_exhaustive():
    """The rANS-W encoder divides by a 32-bit fixed-point reciprocal (csrc/sicn_codec.hip: ransw_div). The library
    checks that very function on the host for EVERY frequency 1..4096 over the states an encoder lane can hold
    (x in [2^16, f << 20)): neighbourhoods of multiples of f across the range, both ends, every power of two.
    Round 1's float reciprocal failed this for 295 frequencies (e.g. f = 3815, x = 250046544)."""
    from simple_image_compression_network_amd import _lib
    n = ctypes.c_ulonglong(0)
    assert _lib.lib().sicn_codec_selftest_div(1, 4097, ctypes.byref(n)) == 0
    assert n.value > 4096 * 50_000
    # and the same arithmetic restated in numpy for the advisor's counterexample and its neighbours
    for f, x in ((3815, 250046544), (181, 181 << 19), (343, 343 * 70001), (405, 405 * 1000003)):
        m = min(0xFFFFFFFF, (1 << 32) // f)
        for xx in range(x - 3, x + 4):
            q = (xx * m) >> 32
            assert q in (xx // f, xx // f - 1) and q <= xx // f


def _skewed_latent(rng, n, dominant_p, mid=(300, 1000)):
    """One dominant symbol with 12-bit frequency ~ dominant_p * 4096 (3700..4095 hits the reciprocals the float
    estimate got wrong), a few mid-frequency symbols, a tail of rare ones."""
    p = np.zeros(128)
    p[0] = dominant_p
    rest = 1.0 - dominant_p
    mids = rng.choice(np.arange(1, 128), 4, replace=False)
    p[mids] = rest * 0.7 / 4
    others = np.setdiff1d(np.arange(1, 128), mids)
    p[others] = rest * 0.3 / others.size
    return rng.choice(128, n, p=p / p.sum()).astype(np.uint8)


def _scaled_latent(rng, shape):
    """A latent whose spread follows a scale map (what a trained hyperprior delivers): s uniform on 0..127, y one-sided
    with mean ~ s/8 — plus the scale map itself."""
    s = rng.integers(0, 128, shape, dtype=np.uint8)
    y = np.minimum((rng.exponential(1.0, shape) * (s.astype(float) / 8 + 0.5)).astype(np.int64), 127).astype(np.uint8)
    return y, s


CTX_SHAPES = [(16, 16, 192), (1, 1, 4), (3, 5, 8), (135, 24, 16), (9, 10, 192), (2, 1, 4), (1, 2, 4), (7, 7, 12), (68, 1, 192)]


@pytest.mark.parametrize("shape", CTX_SHAPES + [(68, 120, 192)])
def test_ctx_oracle_round_trip_and_model_gain(shape):
    """Mode 4 (hyperprior + checkerboard context; oracle/sicn_hyper_oracle.c): decode(encode(y, s), s) == y for even / odd
    widths and heights, single rows / columns; on a latent that really follows its scale map the conditional model beats
    the single static table of mode 3 once the 3.8 KB of extra tables are paid for."""
    rng = np.random.default_rng(sum(shape))
    y, s = _scaled_latent(rng, shape)
    blob = c_oracle.ctx_encode(y, s, (shape[1] * 16, shape[0] * 16))
    back, info = c_oracle.ctx_decode(blob, s)
    assert np.array_equal(back, y) and info.tolist()[:6] == [4, shape[1] * 16, shape[0] * 16, shape[1], shape[0], shape[2]]
    with pytest.raises(RuntimeError):
        c_oracle.ctx_decode(blob[:-2] + bytes([blob[-2] ^ 0x10, blob[-1]]), s)
    if y.size > 1000000:
        assert len(blob) < 0.97 * len(c_oracle.codec_encode(y, (0, 0), 3))
    # the model is conditional: another scale map no longer decodes the same container
    if y.size > 1000:
        try:
            other, _ = c_oracle.ctx_decode(blob, np.roll(s, 1, axis=2))
            assert not np.array_equal(other, y)
        except RuntimeError:
            pass


# ------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("shape", [c for c in CTX_SHAPES if c[2] % 4 == 0] + [(135, 240, 192)])
def test_gpu_ctx_container_equals_oracle_and_round_trips(shape):
    import torch
    from simple_image_compression_network_amd import codec
    rng = np.random.default_rng(sum(shape) + 5)
    n_img = 3 if np.prod(shape) < 1e6 else 1
    ys, ss = zip(*[_scaled_latent(rng, shape) for _ in range(n_img)])
    y, s = np.stack(ys), np.stack(ss)
    yd, sd = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()
    coder = codec.ContextCoder(n_img, *shape, image_width=shape[1] * 16, image_height=shape[0] * 16)
    coder.encode(yd, sd)
    back = torch.full_like(yd, 77)
    coder.decode(back, sd)
    coder.check()
    sizes = coder.sizes()
    for i in range(n_img):
        blob = coder.slots[i, :sizes[i]].cpu().numpy().tobytes()
        assert blob == c_oracle.ctx_encode(y[i], s[i], (shape[1] * 16, shape[0] * 16)), i
    assert torch.equal(back, yd)
    # the GPU decoder accepts what the CPU coder wrote, and reports a wrong scale map / a corrupted payload
    if n_img > 1:
        bad_s = sd.clone()
        bad_s[1] = torch.roll(sd[1], 1, dims=2)
        coder.decode(back, bad_s)
        st = coder.dec_status.cpu().numpy()
        assert st[0, 0] == 0 and st[2, 0] == 0 and (st[1, 0] != 0 or shape[0] * shape[1] * shape[2] < 64)
        corrupt = coder.slots.clone()
        corrupt[0, sizes[0] - 3] ^= 0x04
        coder.decode(back, sd, slots=corrupt)
        assert coder.dec_status[0, 0].item() != 0 and coder.dec_status[1, 0].item() == 0
        bad_y = yd.clone()
        bad_y[2, 0, 0, 0] = 200
        coder.encode(bad_y, sd)
        st = coder.enc_status.cpu().numpy()
        assert st[2, 0] & 1 and st[0, 0] == 0


@gpu
@pytest.mark.parametrize("dominant_p", [0.905, 0.9313, 0.96, 0.99, 0.999, 0.08, 0.25])
def test_gpu_ransw_equals_oracle_on_skewed_latents(dominant_p):
    """>= 4 M symbols per case, dominant frequencies 3700..4095 and mid frequencies 300..1000: the GPU container
    must equal the oracle's (exact x / f) byte for byte and decode back (float reciprocal overshoot)."""
    import torch
    from simple_image_compression_network_amd import codec
    rng = np.random.default_rng(int(dominant_p * 1e4))
    n = 135 * 240 * 192 if dominant_p < 0.9 else 4 * 1024 * 1024 + 12345
    sym = _skewed_latent(rng, n, dominant_p) if dominant_p >= 0.9 else np.minimum(
        rng.geometric(dominant_p, n) - 1, 127).astype(np.uint8)        # natural-like: geometric magnitudes
    lat = sym.reshape(1, 1, -1) if dominant_p >= 0.9 else sym.reshape(135, 240, 192)
    dev = torch.from_numpy(lat).cuda()
    blob = codec.encode_latent(dev, 0, 0, codec.RANSW)
    ref = c_oracle.codec_encode(lat, (0, 0), 3)
    assert blob.cpu().numpy().tobytes() == ref
    back, _ = codec.decode_latent(blob)
    assert torch.equal(back, dev)


@gpu
def test_gpu_decode_rejects_hostile_length_tables():
    """The per-stream length table is untrusted: entries that are huge, that wrap a 32-bit sum back onto
    payload_bytes, or that point past the payload must give SICN_EINVAL (never a GPU fault), in the single and
    in the batch path."""
    import torch
    from simple_image_compression_network_amd import _lib, codec
    rng = np.random.default_rng(33)
    lat = np.stack([_mock_latent(rng, (9, 10, 192)) for _ in range(3)])    # 17280 symbols: 2 wave streams each
    dev = torch.from_numpy(lat).cuda()
    slots, sizes = codec.encode_latents(dev, 160, 144)
    tab = 48 + 256                                                          # offset of the u32 length table
    good = slots[1, tab:tab + 8].cpu().numpy().copy().view("<u4")
    pb = int(good.sum())

    def patched(entries):
        s = slots.clone()
        s[1, tab:tab + 8] = torch.from_numpy(np.array(entries, "<u4").view(np.uint8).copy()).cuda()
        return s

    hostile = [[0xFFFF0000, (pb - 0xFFFF0000) % (1 << 32)],     # wraps to payload_bytes mod 2^32
               [0xFFFFFFFF, 1 + pb], [pb + 2, 0xFFFFFFFE], [int(good[0]), 0x40000000], [0x7FFFFFF0, 0x7FFFFFF0],
               [int(good[0]) + 2, int(good[1]) - 2]]               # plausible sizes, wrong split
    for entries in hostile:
        bad = patched(entries)
        with pytest.raises(_lib.SicnError) as e:
            codec.decode_latents(bad, sizes)
        assert e.value.code in (-22, -74), entries
        with pytest.raises(_lib.SicnError) as e:
            codec.decode_latent(bad[1, :sizes[1]].clone())
        assert e.value.code in (-22, -74), entries
    back, _ = codec.decode_latents(slots, sizes)                             # the device still works afterwards
    assert torch.equal(back, dev)


@gpu
@pytest.mark.parametrize("shape", SHAPES + [(135, 240, 192)])
def test_gpu_container_equals_oracle_and_round_trips(shape):
    import torch
    from simple_image_compression_network_amd import codec
    rng = np.random.default_rng(sum(shape))
    lat = _mock_latent(rng, shape)
    dev = torch.from_numpy(lat).cuda()
    for mode in (codec.RAW8, codec.PACKED7, codec.RANS, codec.RANSW):
        blob = codec.encode_latent(dev, shape[1] * 16, shape[0] * 16, mode)
        host = blob.cpu().numpy().tobytes()
        assert host == c_oracle.codec_encode(lat, (shape[1] * 16, shape[0] * 16), mode), f"mode {mode}"
        back, info = codec.decode_latent(blob)
        assert torch.equal(back, dev) and info.mode == mode
        # and the GPU decoder accepts what the CPU coder wrote
        back2, _ = codec.decode_latent(torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda())
        assert torch.equal(back2, dev)


@gpu
def test_gpu_codec_on_real_latent_and_errors():
    import torch
    from simple_image_compression_network_amd import _lib, api, codec
    x = np.random.default_rng(0).integers(0, 256, (1, 512, 768, 3), dtype=np.uint8)
    net = api.EightLayersNet(768, 512)
    _, latent = net.forward(torch.from_numpy(x).cuda())
    for mode in (codec.RANS, codec.RANSW):
        blob = codec.encode_latent(latent[0], 768, 512, mode)
        back, info = codec.decode_latent(blob)
        assert torch.equal(back, latent[0]) and info.mode == mode
    assert (info.lat_w, info.lat_h, info.lat_c, info.image_width) == (48, 32, 192, 768)
    assert blob.numel() < latent[0].numel()                 # order-0 entropy of this latent is ~4.5 bit/symbol
    # decoding the decoded latent's reconstruction is the same as without the codec in between
    out_a, _ = net.run_layers(4, 7, latent)
    out_b, _ = net.run_layers(4, 7, back[None])
    assert torch.equal(out_a, out_b)
    bad = latent[0].clone()
    bad[0, 0, 0] = 200                                       # symbol >= 128
    with pytest.raises(_lib.SicnError) as e:
        codec.encode_latent(bad, 768, 512, codec.RANS)
    assert e.value.code == -22
    corrupt = blob.clone()
    corrupt[-7] ^= 0x10
    with pytest.raises(_lib.SicnError) as e:
        codec.decode_latent(corrupt)
    assert e.value.code in (-22, -74)


@gpu
def test_gpu_batch_equals_single_calls_and_oracle():
    """sicn_codec_encode_batch / decode_batch: container i is byte-identical to the single-image call and to the
    oracle; decode_batch inverts it; a corrupted member is reported."""
    import torch
    from simple_image_compression_network_amd import _lib, codec
    rng = np.random.default_rng(21)
    lat = np.stack([_mock_latent(rng, (9, 10, 192), zero_frac=z) for z in (0.5, 0.1, 0.9, 0.0, 1.0)])
    dev = torch.from_numpy(lat).cuda()
    slots, sizes = codec.encode_latents(dev, 160, 144)
    for i in range(lat.shape[0]):
        blob = slots[i, :sizes[i]].cpu().numpy().tobytes()
        assert blob == c_oracle.codec_encode(lat[i], (160, 144), 3)
        assert blob == codec.encode_latent(dev[i], 160, 144, codec.RANSW).cpu().numpy().tobytes()
    back, infos = codec.decode_latents(slots, sizes)
    assert torch.equal(back, dev) and all(i.mode == 3 and i.lat_c == 192 for i in infos)
    bad = slots.clone()
    bad[2, sizes[2] - 3] ^= 0x04
    with pytest.raises(_lib.SicnError) as e:
        codec.decode_latents(bad, sizes)
    assert e.value.code in (-22, -74)


@gpu
def test_gpu_async_pair_equals_sync_and_oracle():
    """sicn_codec_encode_batch_async / decode_batch_async: device-side statistics -> normalisation -> header; containers
    byte-identical to the synchronous calls and to the oracle on distributions that stress the normalisation walk
    (many rare symbols: the sum of floors overshoots 4096 and several entries are corrected), sizes and verdicts in
    device memory, decode round trip exact."""
    import torch
    from simple_image_compression_network_amd import codec
    rng = np.random.default_rng(77)
    shape = (9, 10, 192)
    n = int(np.prod(shape))
    lats = [_mock_latent(rng, shape, zero_frac=z) for z in (0.5, 0.0, 1.0)]
    # many rare symbols: 127 symbols appear 1-3 times each beside one dominant -> every rare v == 0 is bumped to 1
    rare = np.zeros(n, np.uint8)
    idx = rng.choice(n, 250, replace=False)
    rare[idx] = rng.integers(1, 128, 250)
    lats.append(rare.reshape(shape))
    lats.append(_skewed_latent(rng, n, 0.9313).reshape(shape))
    lat = np.stack(lats)
    dev = torch.from_numpy(lat).cuda()
    coder = codec.LatentCoder(lat.shape[0], *shape, image_width=160, image_height=144, stream_symbols=16384)   # what the synchronous calls use
    coder.encode(dev)
    back = torch.empty_like(dev)
    coder.decode(back)
    coder.check()
    sizes = coder.sizes()
    for i in range(lat.shape[0]):
        blob = coder.slots[i, :sizes[i]].cpu().numpy().tobytes()
        assert blob == c_oracle.codec_encode(lat[i], (160, 144), 3), i
    assert torch.equal(back, dev)
    # the synchronous wrappers give the same bytes
    slots, sz = codec.encode_latents(dev, 160, 144)
    assert sz == sizes and all(torch.equal(slots[i, :sz[i]], coder.slots[i, :sz[i]]) for i in range(len(sz)))


@gpu
@pytest.mark.parametrize("ss", [1024, 4096, 8192, "auto"])
def test_gpu_stream_length_parameter_equals_oracle(ss):
    """sicn_codec_*_batch_async_sl: containers byte-identical to the oracle's at the same stream length, round trip exact; the
    synchronous decoders read the length from the header; a decoder told another length reports the mismatch (bit 2)."""
    import torch
    from simple_image_compression_network_amd import codec
    rng = np.random.default_rng(91)
    shape = (17, 30, 192)                                   # 97920 symbols: 6 streams of 16384 ... 96 of 1024
    lat = np.stack([_mock_latent(rng, shape, zero_frac=z) for z in (0.5, 0.1, 0.97)])
    dev = torch.from_numpy(lat).cuda()
    coder = codec.LatentCoder(3, *shape, image_width=480, image_height=272, stream_symbols=ss)
    if ss == "auto":
        assert coder.stream_symbols == codec.auto_stream_symbols(lat[0].size, 3) == 8192
    ssv = coder.stream_symbols
    coder.encode(dev)
    back = torch.empty_like(dev)
    coder.decode(back)
    coder.check()
    assert torch.equal(back, dev)
    sizes = coder.sizes()
    for i in range(3):
        blob = coder.slots[i, :sizes[i]].cpu().numpy().tobytes()
        assert blob == c_oracle.codec_encode(lat[i], (480, 272), 3, stream_symbols=ssv), i
        got, info = codec.decode_latent(coder.slots[i, :sizes[i]].clone())          # synchronous single-container decoder
        assert int(info.stream_symbols) == ssv and np.array_equal(got.cpu().numpy(), lat[i])
    lats, infos = codec.decode_latents(coder.slots, sizes)                            # synchronous batch decoder
    assert torch.equal(lats, dev) and all(int(f.stream_symbols) == ssv for f in infos)
    # the oracle's containers go through the GPU decoder too
    other = codec.LatentCoder(3, *shape, stream_symbols=ssv)
    slots = torch.zeros_like(other.slots)
    for i in range(3):
        b = np.frombuffer(c_oracle.codec_encode(lat[i], (1, 2), 3, stream_symbols=ssv), np.uint8)
        slots[i, :b.size] = torch.from_numpy(b.copy()).cuda()
    back.zero_()
    other.decode(back, slots=slots)
    other.check()
    assert torch.equal(back, dev)
    # a decoder built for another stream length rejects the containers instead of misreading them
    wrong = codec.LatentCoder(3, *shape, stream_symbols=16384 if ssv != 16384 else 4096)
    w_slots = torch.zeros_like(wrong.slots)
    k = min(w_slots.shape[1], coder.slots.shape[1])
    w_slots[:, :k] = coder.slots[:, :k]
    wrong.decode(back, slots=w_slots)
    st = wrong.dec_status.cpu().numpy()
    assert all(st[i, 0] & 4 for i in range(3)), st


@gpu
def test_gpu_async_decode_with_many_streams_takes_the_scan_path():
    """More than 2048 streams per image (here 2160 of 1024 symbols): the asynchronous decoder goes back to its four-kernel form
    (parse, scan, streams, finish) — up to 2048 every wave sums the length table itself.  Same bytes, same verdicts."""
    import torch
    from simple_image_compression_network_amd import _lib, codec
    shape = (64, 180, 192)
    lat = _mock_latent(np.random.default_rng(93), (2,) + shape)
    dev = torch.from_numpy(lat).cuda()
    coder = codec.LatentCoder(2, *shape, stream_symbols=1024)
    coder.encode(dev)
    back = torch.empty_like(dev)
    coder.decode(back)
    coder.check()
    assert torch.equal(back, dev)
    sizes = coder.sizes()
    assert coder.slots[1, :sizes[1]].cpu().numpy().tobytes() == c_oracle.codec_encode(lat[1], (0, 0), 3, stream_symbols=1024)
    bad = coder.slots.clone()
    bad[0, 48 + 256 + 4 * 2100 + 2] ^= 0x7F                 # length entry of stream 2100 of image 0: far above the cap
    coder.decode(back, slots=bad)
    st = coder.dec_status.cpu().numpy()
    assert st[0, 0] & 32 and st[1, 0] == 0, st
    with pytest.raises(_lib.SicnError):
        coder.check()


@gpu
@pytest.mark.parametrize("n_streams", [2048, 2049])
def test_gpu_form_boundary_through_every_entry_point(n_streams):
    """2048 streams of 1024 symbols is the last size of the self-scanning form, 2049 the first of the scan form (parse, scan,
    streams, finish).  On both sides of it the asynchronous encoder writes the oracle's bytes, the asynchronous decoder and the
    synchronous single-container decoder — a batch of one through the same launches — round-trip, and a hostile length-table
    entry is SICN_EINVAL from the synchronous decoder."""
    import torch
    from simple_image_compression_network_amd import _lib, codec
    shape = (1, 2048 * 1024 + (n_streams - 2048), 1)
    lat = _mock_latent(np.random.default_rng(n_streams), shape)
    dev = torch.from_numpy(lat).cuda()
    coder = codec.LatentCoder(1, *shape, stream_symbols=1024)
    coder.encode(dev[None])
    back = torch.empty_like(dev[None])
    coder.decode(back)
    coder.check()
    assert torch.equal(back[0], dev)
    blob = coder.slots[0, :coder.sizes()[0]].clone()
    assert blob.cpu().numpy().tobytes() == c_oracle.codec_encode(lat, (0, 0), 3, stream_symbols=1024)
    got, info = codec.decode_latent(blob)
    assert int(info.n_streams) == n_streams and int(info.stream_symbols) == 1024 and torch.equal(got, dev)
    bad = blob.clone()
    bad[48 + 256 + 4 * (n_streams - 3) + 2] ^= 0x7F         # one length entry far above the cap of 2304 bytes
    with pytest.raises(_lib.SicnError) as e:
        codec.decode_latent(bad)
    assert e.value.code == -22


@gpu
@pytest.mark.parametrize("shape", [(1, 1, 65), (9, 10, 192), (0, 4, 4)])
def test_gpu_sync_encode_equals_oracle_and_async_pair(shape):
    """codec.encode_latent in mode 3 is the asynchronous encoder with one image at the default stream length: the oracle's bytes
    and LatentCoder's, byte for byte (one short stream, two streams, the empty latent); a symbol >= 128 is SICN_EINVAL."""
    import torch
    from simple_image_compression_network_amd import _lib, codec
    lat = _mock_latent(np.random.default_rng(7 + sum(shape)), shape)
    dev = torch.from_numpy(lat).cuda()
    wh = (shape[1] * 16, shape[0] * 16)
    blob = codec.encode_latent(dev, *wh, codec.RANSW).cpu().numpy().tobytes()
    assert blob == c_oracle.codec_encode(lat, wh, 3)
    coder = codec.LatentCoder(1, *shape, image_width=wh[0], image_height=wh[1], stream_symbols=16384)
    coder.encode(dev[None])
    coder.check()
    assert blob == coder.slots[0, :coder.sizes()[0]].cpu().numpy().tobytes()
    if lat.size == 0:
        assert len(blob) == 304
        return
    bad = dev.clone()
    bad.view(-1)[lat.size // 2] = 200
    with pytest.raises(_lib.SicnError) as e:
        codec.encode_latent(bad, *wh, codec.RANSW)
    assert e.value.code == -22


@gpu
def test_gpu_async_reports_errors_in_device_status():
    import torch
    from simple_image_compression_network_amd import _lib, codec
    rng = np.random.default_rng(78)
    shape = (9, 10, 192)
    lat = np.stack([_mock_latent(rng, shape) for _ in range(3)])
    dev = torch.from_numpy(lat).cuda()
    coder = codec.LatentCoder(3, *shape)
    bad = dev.clone()
    bad[1, 0, 0, 0] = 200                                     # symbol >= 128 in image 1 only
    coder.encode(bad)
    st = coder.enc_status.cpu().numpy()
    assert st[1, 0] & 1 and st[0, 0] == 0 and st[2, 0] == 0
    coder.encode(dev)
    assert not coder.enc_status[:, 0].any()
    sizes = coder.sizes()
    back = torch.empty_like(dev)
    good = coder.slots.clone()
    # payload bit flip -> stream error or checksum; header shape mismatch; frequency table sum; hostile table; short slot
    cases = []
    c = good.clone(); c[0, sizes[0] - 3] ^= 0x04; cases.append((c, None, 0))
    c = good.clone(); c[2, 16] ^= 0x01; cases.append((c, None, 2))                 # lat_w field
    c = good.clone(); c[1, 48 + 7] ^= 0x01; cases.append((c, None, 1))             # a frequency
    tab = 48 + 256
    c = good.clone(); c[1, tab:tab + 4] = torch.tensor([0, 0, 255, 255], dtype=torch.uint8).cuda(); cases.append((c, None, 1))
    short = coder.enc_status.clone(); short[2, 1] = 100; cases.append((good.clone(), short, 2))
    for slots, valid, which in cases:
        coder.decode(back, slots=slots, valid=valid)
        st = coder.dec_status.cpu().numpy()
        assert st[which, 0] != 0, (which, st)
        assert all(st[k, 0] == 0 for k in range(3) if k != which), st
        with pytest.raises(_lib.SicnError):
            coder.check()
    coder.decode(back, slots=good)
    coder.check()
    assert torch.equal(back, dev)


@gpu
def test_gpu_coded_pipeline_is_graph_capturable():
    """analysis -> encode -> decode -> synthesis as ONE hipGraph: none of the four stages allocates or synchronises."""
    import gc
    import torch
    from simple_image_compression_network_amd import api, codec
    net = api.EightLayersNet(256, 256)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.integers(0, 256, (2, 256, 256, 3), dtype=np.uint8)).cuda()
    lat, lat2 = (torch.empty((2, 16, 16, 192), dtype=torch.uint8, device="cuda") for _ in range(2))
    out = torch.empty((2, 256, 256, 3), dtype=torch.uint8, device="cuda")
    coder = codec.LatentCoder(2, 16, 16, 192, 256, 256)

    def pipeline():
        net.analysis(x, lat)
        coder.encode(lat)
        coder.decode(lat2)
        net.synthesis(lat2, out)

    pipeline()
    coder.check()
    ref_out, _ = net.forward(x)
    torch.cuda.synchronize()
    assert torch.equal(out, ref_out)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                pipeline()
    finally:
        gc.enable()
    x.copy_(torch.from_numpy(rng.integers(0, 256, (2, 256, 256, 3), dtype=np.uint8)).cuda())
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    coder.check()
    ref_out, ref_lat = net.forward(x)
    torch.cuda.synchronize()
    assert torch.equal(out, ref_out) and torch.equal(lat2, ref_lat)


@gpu
def test_gpu_1080p_sized_container_equals_oracle_at_the_auto_stream_length():
    """BASELINE.json configs[2] includes the coder: a container of the 1080p latent's size (68 x 120 x 192 = 1.57 M symbols, 192
    streams at the automatic length of 8192) byte-identical to the oracle's, round trip exact (on the GPU that
    size used to be covered by round trip + transform hashes only)."""
    import torch
    from simple_image_compression_network_amd import codec
    rng = np.random.default_rng(1080)
    shape = (68, 120, 192)
    lat = np.stack([_mock_latent(rng, shape, zero_frac=0.5)])
    dev = torch.from_numpy(lat).cuda()
    coder = codec.LatentCoder(1, *shape, image_width=1920, image_height=1080)      # default = "auto"
    assert coder.stream_symbols == 8192
    coder.encode(dev)
    back = torch.empty_like(dev)
    coder.decode(back)
    coder.check()
    assert torch.equal(back, dev)
    size = coder.sizes()[0]
    blob = coder.slots[0, :size].cpu().numpy().tobytes()
    ref = c_oracle.codec_encode(lat[0], (1920, 1080), 3, stream_symbols=8192)
    assert blob == ref
    got, info = codec.decode_latent(coder.slots[0, :size].clone())
    assert int(info.stream_symbols) == 8192 and int(info.n_streams) == 192 and np.array_equal(got.cpu().numpy(), lat[0])


@gpu
def test_gpu_decoder_built_from_the_container_header():
    """a default LatentCoder (automatic stream length: 8192 for a 1080p latent) cannot decode containers written with another
    length — e.g. by the C entry points without `_sl`, which always write 16384-symbol streams: the decode reports status bit 2.
    LatentCoder.for_containers reads shape and stream length from the header and decodes them."""
    import torch
    from simple_image_compression_network_amd import _lib, codec
    rng = np.random.default_rng(77)
    shape = (68, 120, 192)
    lat = np.stack([_mock_latent(rng, shape, zero_frac=0.5) for _ in range(2)])
    dev = torch.from_numpy(lat).cuda()
    slots, sizes = codec.encode_latents(dev, 1920, 1080)                 # sicn_codec_encode_batch: the format's default length
    assert int(codec.parse_header(bytes(slots[0, :48].cpu().numpy().tobytes())).stream_symbols) == 16384
    dec = codec.LatentCoder.for_containers(slots)
    assert dec.stream_symbols == 16384 and dec.shape == (2,) + shape and dec.image_wh == (1920, 1080)
    back = torch.empty_like(dev)
    dec.decode(back, slots=slots)
    dec.check()
    assert torch.equal(back, dev)
    # the adopted object encodes into a buffer of ITS slot size (the writer's), byte-identical to what it was given
    dec.encode(dev)
    dec.check()
    assert dec.sizes() == sizes and all(torch.equal(dec.slots[i, :sizes[i]], slots[i, :sizes[i]]) for i in range(2))
    # and the mismatch the factory exists to prevent: the automatic decoder on the same containers
    auto = codec.LatentCoder(2, *shape)
    assert auto.stream_symbols == 8192
    if auto.slot <= int(slots.shape[1]):
        padded = torch.zeros((2, auto.slot), dtype=torch.uint8, device="cuda")
        padded[:, :min(auto.slot, int(slots.shape[1]))] = slots[:, :auto.slot]
        auto.decode(torch.empty_like(dev), slots=padded)
        with pytest.raises(_lib.SicnError):
            auto.check()
