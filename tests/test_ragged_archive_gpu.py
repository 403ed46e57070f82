"""GPU checks of the ragged archive (include/sicn_ragged_archive.h, csrc/k_ragged_archive.hip; run with -m gpu on an MI355X): the
containers of a batch packed into one "SICA" byte string with two launches and unpacked with two.  Everything is byte equality against
the numpy statement of the format in tests/archive_cases.py.  Most cases drive the C entry points with synthetic slot buffers (random
bytes) and synthetic status arrays — the kernels do not look inside a container, and the archive object is generic over slot layouts —
the last ones go through the real coders, the net and the hyperprior codec."""
import ctypes

import numpy as np
import pytest

import archive_cases as ac

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL, ENOSPC = -22, -28
GUARD = 256
OUT_PATTERN, SLOT_PATTERN = 0xEE, 0x5A
U64P = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def codec(lib):
    from simple_image_compression_network_amd import codec as _codec
    return _codec


def _chunk(lib):
    return int(lib.lib().sicn_ragged_archive_chunk_bytes())


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Synthetic:
    """An archive object over k synthetic sections of n slots: caps[i][s] bytes each, back to back at multiples of 16 (plus a gap
    here and there), random slot bytes, status arrays {0, sizes[i][s]}.  `odd`: every slot buffer is a view that begins `odd`
    bytes into its allocation — not a multiple of 16, so the byte path runs."""

    def __init__(self, lib, sizes, caps, seed=0, odd=0):
        self.lib, self.L = lib, lib.lib()
        self.sizes, self.caps = np.asarray(sizes, dtype=np.int64), np.asarray(caps, dtype=np.int64)
        self.n, self.k = self.sizes.shape
        assert self.caps.shape == (self.n, self.k)
        rng = np.random.default_rng(seed)
        self.off, self.host, self.slots, self.status = [], [], [], []
        for s in range(self.k):
            at, offs = 0, []
            for i in range(self.n):
                offs.append(at)
                at += ac.a16(self.caps[i, s]) + 16 * ((i + s) % 3 == 0)
            self.off.append(offs)
            host = rng.integers(0, 256, max(at, 16), dtype=np.uint8)
            self.host.append(host)
            base = torch.empty(host.size + 16, dtype=torch.uint8, device="cuda")
            view = base[odd:odd + host.size]
            view.copy_(torch.from_numpy(host))
            assert view.data_ptr() % 16 == odd % 16
            self.slots.append(view)
            self.status.append(_dev(np.stack([np.zeros(self.n, np.int32), self.sizes[:, s].astype(np.uint32).view(np.int32)], axis=1)))
        self._tables = [(ctypes.c_uint64 * self.n)(*offs) for offs in self.off], \
                       [(ctypes.c_uint64 * self.n)(*[int(v) for v in self.caps[:, s]]) for s in range(self.k)]
        pp = U64P * self.k
        self.h = ctypes.c_void_p()
        rc = self.L.sicn_ragged_archive_create(self.n, self.k, pp(*[ctypes.cast(a, U64P) for a in self._tables[0]]),
                                               pp(*[ctypes.cast(a, U64P) for a in self._tables[1]]), ctypes.byref(self.h))
        assert rc == 0, rc
        self.max_bytes = int(self.L.sicn_ragged_archive_max_bytes(self.h))
        self.ws = torch.empty(max(int(self.L.sicn_ragged_archive_workspace_bytes(self.h)), 16), dtype=torch.uint8, device="cuda")
        self.st = torch.zeros(4, dtype=torch.int32, device="cuda")

    def __del__(self):
        if getattr(self, "h", None):
            self.L.sicn_ragged_archive_free(self.h)
            self.h = None

    def containers(self, sizes=None):
        sizes = self.sizes if sizes is None else np.asarray(sizes)
        return [tuple(self.host[s][self.off[s][i]:self.off[s][i] + int(sizes[i, s])].tobytes() for s in range(self.k)) for i in range(self.n)]

    def ptrs(self, tensors):
        return (ctypes.c_void_p * self.k)(*[t.data_ptr() for t in tensors])

    def read_status(self):
        torch.cuda.synchronize()
        e, bad, lo, hi = (int(v) & 0xFFFFFFFF for v in self.st.cpu().tolist())
        return e, bad, lo | hi << 32

    def pack(self, tag, out, capacity=None, ws_bytes=None, status=None):
        return self.L.sicn_ragged_archive_pack_async(self.h, self.ptrs(self.slots), self.ptrs(status or self.status), tag, _vp(out),
                                                     out.numel() if capacity is None else capacity, _vp(self.st), _vp(self.ws),
                                                     self.ws.numel() if ws_bytes is None else ws_bytes, None)

    def guarded_out(self, odd=0):
        """(whole allocation filled with OUT_PATTERN, the view handed to pack: max_bytes + 64 bytes behind a guard band)."""
        whole = torch.full((GUARD + self.max_bytes + 64 + GUARD + 16,), OUT_PATTERN, dtype=torch.uint8, device="cuda")
        return whole, whole[GUARD + odd:GUARD + odd + self.max_bytes + 64]

    def check_pack(self, tag=0x1234ABCD, odd=0, sizes=None, want_error=0, want_bad=ac.NO_ENTRY):
        """pack -> the archive; asserts it is the numpy statement's, byte for byte, and that no byte outside it was written."""
        want = ac.make_archive(self.containers(sizes), tag)
        whole, out = self.guarded_out(odd)
        assert out.data_ptr() % 16 == odd % 16
        assert self.pack(tag, out) == 0
        e, bad, nbytes = self.read_status()
        assert (e, bad, nbytes) == (want_error, want_bad, len(want))
        assert nbytes <= self.max_bytes
        host = whole.cpu().numpy()
        a = GUARD + odd
        got = host[a:a + nbytes].tobytes()
        if got != want:
            first = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError(f"archive differs from the numpy statement at byte {first} of {len(want)}")
        assert (host[:a] == OUT_PATTERN).all(), "the guard band in front of the archive buffer was written"
        assert (host[a + nbytes:] == OUT_PATTERN).all(), "bytes behind total_bytes were written"
        return want

    def check_unpack(self, archive: bytes, tag=0x1234ABCD, odd=0, sizes=None, n_in=None):
        """unpack into slot buffers pre-filled with a pattern: the containers are restored, every other byte still holds the pattern,
        the valid arrays hold {0, size}."""
        sizes = self.sizes if sizes is None else np.asarray(sizes)
        base = torch.empty(len(archive) + 32, dtype=torch.uint8, device="cuda")
        src = base[odd:odd + len(archive)]
        src.copy_(torch.frombuffer(bytearray(archive), dtype=torch.uint8))
        for t in self.slots:
            t.fill_(SLOT_PATTERN)
        valid = [torch.full((self.n, 2), -1, dtype=torch.int32, device="cuda") for _ in range(self.k)]
        rc = self.L.sicn_ragged_archive_unpack_async(self.h, _vp(src), len(archive) if n_in is None else n_in, tag, self.ptrs(self.slots),
                                                     self.ptrs(valid), _vp(self.st), _vp(self.ws), self.ws.numel(), None)
        assert rc == 0
        e, bad, nbytes = self.read_status()
        assert (e, bad, nbytes) == (0, ac.NO_ENTRY, len(archive))
        for s in range(self.k):
            want = np.full(self.host[s].size, SLOT_PATTERN, np.uint8)
            for i in range(self.n):
                o, z = self.off[s][i], int(sizes[i, s])
                want[o:o + z] = self.host[s][o:o + z]
            got = self.slots[s].cpu().numpy()
            assert np.array_equal(got, want), f"section {s}: byte {int(np.flatnonzero(got != want)[0])} of the slot buffer"
            assert np.array_equal(valid[s].cpu().numpy().astype(np.int64), np.stack([np.zeros(self.n, np.int64), sizes[:, s]], axis=1))


def _edge_case(lib, k, seed, odd=0):
    """Sizes around the 16-byte vector and the chunk, one entry that fills its slot; capacities differ per entry."""
    c = _chunk(lib)
    edge = [0, 1, 15, 16, 17, c - 1, c, c + 1, 2 * c + 5, 3 * c + 7]
    n = len(edge)
    sizes = np.array([[edge[(i + 3 * s) % n] for s in range(k)] for i in range(n)])
    caps = np.array([[sizes[i, s] if sizes[i, s] == 3 * c + 7 else sizes[i, s] + 1 + 37 * ((i + s) % 4) for s in range(k)] for i in range(n)])
    return Synthetic(lib, sizes, caps, seed=seed, odd=odd)


# ---- 1 - 3: chunk and vector edges, sections, the byte path; 5: the round trip of each --------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 4])
def test_chunk_and_vector_edges_pack_and_round_trip(lib, k):
    syn = _edge_case(lib, k, seed=40 + k)
    assert int(lib.lib().sicn_ragged_archive_max_bytes(syn.h)) == ac.layout(syn.caps)[1] >= ac.layout(syn.sizes)[1]
    archive = syn.check_pack()
    syn.check_unpack(archive)


@pytest.mark.parametrize("k,odd_slots,odd_archive", [(1, 1, 3), (2, 3, 1), (2, 0, 1), (2, 3, 0), (4, 1, 3)])
def test_byte_path_gives_the_same_bytes(lib, k, odd_slots, odd_archive):
    """Slot buffers and the archive buffer taken as views at odd offsets: no 16-byte vector is possible, the bytes are the same."""
    syn = _edge_case(lib, k, seed=40 + k, odd=odd_slots)
    aligned = _edge_case(lib, k, seed=40 + k)
    archive = syn.check_pack(odd=odd_archive)
    assert archive == aligned.check_pack()
    syn.check_unpack(archive, odd=odd_archive)


def test_max_bytes_is_the_layout_of_full_slots(lib):
    """max_bytes >= the layout's total when every size is its capacity (equal, by the format's arithmetic), through the C layout too."""
    caps = np.array([[100, 1], [16, 2], [0, 3], [16385, 4], [48, 5]])
    syn = Synthetic(lib, caps, caps, seed=2)
    total = ctypes.c_uint64()
    flat = np.ascontiguousarray(caps, dtype=np.uint32).reshape(-1)
    assert lib.lib().sicn_ragged_archive_layout(flat.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 5, 2, None, ctypes.byref(total)) == 0
    assert syn.max_bytes >= ac.layout(caps)[1] and syn.max_bytes == total.value == ac.layout(caps)[1]
    assert int(lib.lib().sicn_ragged_archive_workspace_bytes(syn.h)) >= 12 * 10
    syn.check_unpack(syn.check_pack())                       # every slot full


# ---- 4: the index scan across passes of the workgroup --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(255, 1), (256, 1), (257, 1), (128, 2), (5000, 2)])
def test_index_scan_across_passes(lib, n, k):
    rng = np.random.default_rng(n)
    sizes = rng.integers(0, 41, (n, k))
    syn = Synthetic(lib, sizes, np.full((n, k), 48), seed=n)
    archive = syn.check_pack(tag=n)
    syn.check_unpack(archive, tag=n)


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------------
def _refusal_object(lib):
    sizes = np.array([[17, 40], [0, 16], [1, 33], [5, 0]])
    syn = Synthetic(lib, sizes, (sizes + 15) // 16 * 16 + 16, seed=6)
    return syn, ac.make_archive(syn.containers(), 9)


def _assert_refused(syn, archive, n_in, tag, bit, want_bad):
    src = torch.empty(max(len(archive), 16), dtype=torch.uint8, device="cuda")
    if archive:
        src[:len(archive)].copy_(torch.frombuffer(bytearray(archive), dtype=torch.uint8))
    for t in syn.slots:
        t.fill_(SLOT_PATTERN)
    valid = [torch.full((syn.n, 2), -1, dtype=torch.int32, device="cuda") for _ in range(syn.k)]
    rc = syn.L.sicn_ragged_archive_unpack_async(syn.h, _vp(src), n_in, tag, syn.ptrs(syn.slots), syn.ptrs(valid), _vp(syn.st), _vp(syn.ws),
                                                syn.ws.numel(), None)
    assert rc == 0
    e, bad, _ = syn.read_status()
    assert e & bit and not e & ~0xF8, f"status {e:#x}, expected bit {bit:#x}"
    assert bad == want_bad
    for s in range(syn.k):
        v = valid[s].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        assert (v[:, 0] == e).all() and (v[:, 1] == 0).all(), "every valid entry of a refused archive is {error, 0}"
        assert (syn.slots[s].cpu().numpy() == SLOT_PATTERN).all(), "a refused archive wrote a slot byte"
    return e


def test_every_refusal_is_clean(lib):
    syn, good = _refusal_object(lib)
    syn.check_unpack(good, tag=9)
    cases = ac.hostile(good, syn.n, syn.k)
    assert {bit for _, _, bit in cases} == {ac.BAD_HEADER, ac.BAD_COUNTS, ac.BAD_SIZE, ac.BAD_TOTAL}
    for name, bad, bit in cases:
        e = _assert_refused(syn, bad, len(bad), 9, bit, 1 if bit == ac.BAD_SIZE else ac.NO_ENTRY)
        if bit in (ac.BAD_HEADER, ac.BAD_COUNTS):
            assert e == bit, name                        # nothing behind a header that cannot be trusted is looked at
    assert _assert_refused(syn, good, len(good), 10, ac.BAD_TAG, ac.NO_ENTRY) == ac.BAD_TAG
    assert _assert_refused(syn, ac.patched(good, 12, "<I", 0x80000009), len(good), 9, ac.BAD_TAG, ac.NO_ENTRY) == ac.BAD_TAG
    # in_bytes shorter than total_bytes — by one byte, by a container, down to a bare header — and shorter than a header
    for n_in in (len(good) - 1, len(good) - 16, 64, 32):
        assert _assert_refused(syn, good[:n_in], n_in, 9, ac.BAD_TOTAL, ac.NO_ENTRY) == ac.BAD_TOTAL
    for n_in in (31, 4, 0):
        assert _assert_refused(syn, good[:n_in], n_in, 9, ac.BAD_HEADER, ac.NO_ENTRY) == ac.BAD_HEADER
    # an index size one byte above its slot's capacity, the total patched with it: bit 6 alone, and the entry is named
    cap5 = int(syn.caps[2, 1])
    over = ac.make_archive([tuple(b"\x01" * (cap5 + 1) if (i, s) == (2, 1) else c for s, c in enumerate(cs)) for i, cs in enumerate(syn.containers())], 9)
    assert _assert_refused(syn, over, len(over), 9, ac.BAD_SIZE, 5) == ac.BAD_SIZE
    # the index's padding (an object of 3 x 2 entries: 8 bytes of it)
    sizes = np.array([[17, 40], [0, 16], [1, 33]])
    padded = Synthetic(lib, sizes, sizes + 16, seed=7)
    good3 = ac.make_archive(padded.containers(), 9)
    padded.check_unpack(good3, tag=9)
    assert _assert_refused(padded, ac.patched(good3, 32 + 28, "<B", 1), len(good3), 9, ac.BAD_HEADER, ac.NO_ENTRY) == ac.BAD_HEADER
    syn.check_unpack(good, tag=9)                            # and the object is as good as before


# ---- 7: pack-side errors --------------------------------------------------------------------------------------------------------------
def test_status_error_and_over_capacity_give_an_empty_entry(lib):
    sizes = np.array([[100, 7], [33, 64], [16, 1], [50, 50], [9, 2000]])
    syn = Synthetic(lib, sizes, sizes + 20, seed=8)
    status = [s.clone() for s in syn.status]
    status[0][2, 0] = 1                                      # image 2, section 0: the encoder reported an error
    status[1][3, 1] = int(syn.caps[3, 1]) + 1                # image 3, section 1: a size above the slot's capacity
    stored = sizes.copy()
    stored[2, 0] = stored[3, 1] = 0
    want = ac.make_archive(syn.containers(stored), 5)
    whole, out = syn.guarded_out()
    assert syn.pack(5, out, status=status) == 0
    assert syn.read_status() == (ac.PACK_STATUS_ERROR | ac.PACK_OVER_CAPACITY, 2 * 2 + 0, len(want))
    assert whole.cpu().numpy()[GUARD:GUARD + len(want)].tobytes() == want
    status[0][2, 0] = 0
    assert syn.pack(5, out, status=status) == 0
    assert syn.read_status()[:2] == (ac.PACK_OVER_CAPACITY, 3 * 2 + 1)


def test_capacity_one_byte_short_and_short_workspace(lib):
    syn = _edge_case(lib, 2, seed=9)
    need = ac.layout(syn.sizes)[1]
    whole, out = syn.guarded_out()
    assert syn.pack(1, out, capacity=need - 1) == 0
    assert syn.read_status() == (ac.PACK_NO_ROOM, ac.NO_ENTRY, need)
    assert (whole.cpu().numpy() == OUT_PATTERN).all(), "bit 2 must leave the output buffer untouched"
    assert syn.pack(1, out, capacity=need) == 0              # exactly enough is enough
    assert syn.read_status() == (0, ac.NO_ENTRY, need)
    assert whole.cpu().numpy()[GUARD:GUARD + need].tobytes() == ac.make_archive(syn.containers(), 1)
    # a short workspace: SICN_ENOSPC and nothing enqueued — neither the status nor the buffer changes
    whole.fill_(OUT_PATTERN)
    syn.st.fill_(-7)
    torch.cuda.synchronize()
    assert syn.pack(1, out, ws_bytes=syn.ws.numel() - 1) == ENOSPC
    need_ws = int(lib.lib().sicn_ragged_archive_workspace_bytes(syn.h))
    assert syn.pack(1, out, ws_bytes=need_ws - 1) == ENOSPC
    valid = [torch.zeros((syn.n, 2), dtype=torch.int32, device="cuda") for _ in range(syn.k)]
    assert syn.L.sicn_ragged_archive_unpack_async(syn.h, _vp(out), out.numel(), 1, syn.ptrs(syn.slots), syn.ptrs(valid), _vp(syn.st),
                                                  _vp(syn.ws), need_ws - 1, None) == ENOSPC
    assert syn.L.sicn_ragged_archive_pack_async(syn.h, syn.ptrs(syn.slots), syn.ptrs(syn.status), 1, None, 0, _vp(syn.st), _vp(syn.ws),
                                                syn.ws.numel(), None) == EINVAL
    torch.cuda.synchronize()
    assert (syn.st.cpu().numpy() == -7).all() and (whole.cpu().numpy() == OUT_PATTERN).all()


# ---- 8: offsets past 2^32 ---------------------------------------------------------------------------------------------------------------
def test_slot_offsets_past_4_gib(lib):
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip(f"the device reports {free >> 20} MiB free: the 4 GiB + 64 KiB slot buffer needs 8 GiB of headroom")
    L = lib.lib()
    c = _chunk(lib)
    offs, caps, sizes = [0, 2 ** 32 + 16], [4096, 2 * c + 64], [1000, c + 21]
    big = torch.empty(2 ** 32 + 65536, dtype=torch.uint8, device="cuda")      # never touched as a whole
    rng = np.random.default_rng(11)
    data = [rng.integers(0, 256, cap, dtype=np.uint8) for cap in caps]
    for o, d in zip(offs, data):
        big[o:o + d.size].copy_(torch.from_numpy(d))
    h = ctypes.c_void_p()
    pp = U64P * 1
    t_off, t_cap = (ctypes.c_uint64 * 2)(*offs), (ctypes.c_uint64 * 2)(*caps)
    assert L.sicn_ragged_archive_create(2, 1, pp(ctypes.cast(t_off, U64P)), pp(ctypes.cast(t_cap, U64P)), ctypes.byref(h)) == 0
    try:
        ws = torch.empty(max(int(L.sicn_ragged_archive_workspace_bytes(h)), 16), dtype=torch.uint8, device="cuda")
        st = torch.zeros(4, dtype=torch.int32, device="cuda")
        status = _dev(np.array([[0, sizes[0]], [0, sizes[1]]], np.int32))
        out = torch.full((int(L.sicn_ragged_archive_max_bytes(h)),), OUT_PATTERN, dtype=torch.uint8, device="cuda")
        one = (ctypes.c_void_p * 1)
        assert L.sicn_ragged_archive_pack_async(h, one(big.data_ptr()), one(status.data_ptr()), 3, _vp(out), out.numel(), _vp(st), _vp(ws),
                                                ws.numel(), None) == 0
        torch.cuda.synchronize()
        want = ac.make_archive([(data[0][:sizes[0]].tobytes(),), (data[1][:sizes[1]].tobytes(),)], 3)
        assert st.cpu().tolist() == [0, -1, len(want), 0]
        assert out.cpu().numpy()[:len(want)].tobytes() == want and (out.cpu().numpy()[len(want):] == OUT_PATTERN).all()
        for o, cap in zip(offs, caps):
            big[o - (16 if o else 0):o + cap + 16].fill_(SLOT_PATTERN)
        valid = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
        assert L.sicn_ragged_archive_unpack_async(h, _vp(out), len(want), 3, one(big.data_ptr()), one(valid.data_ptr()), _vp(st), _vp(ws),
                                                  ws.numel(), None) == 0
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0, -1, len(want), 0] and valid.cpu().tolist() == [[0, sizes[0]], [0, sizes[1]]]
        for o, cap, size, d in zip(offs, caps, sizes, data):
            got = big[o - (16 if o else 0):o + cap + 16].cpu().numpy()
            lead = 16 if o else 0
            assert np.array_equal(got[lead:lead + size], d[:size])
            assert (got[:lead] == SLOT_PATTERN).all() and (got[lead + size:] == SLOT_PATTERN).all()
    finally:
        L.sicn_ragged_archive_free(h)


# ---- 9: the real coders -----------------------------------------------------------------------------------------------------------------
# (lat_w, lat_h, stream_symbols): the 12 mixed shapes of tests/test_ragged_codec.py
SHAPES = [(1, 1, 1024), (3, 7, 16384), (16, 12, 8192), (13, 11, 2048), (2, 9, 4096), (48, 48, 1024), (64, 1, 16384), (1, 64, 1024),
          (31, 17, 2048), (40, 30, 8192), (5, 5, 4096), (120, 68, 16384)]
LAT_C = 192


def _skewed(rng, shape):
    """About half zeros, a geometric tail, values < 128 — what a ReLU latent looks like to the coder."""
    n = int(np.prod(shape))
    x = np.minimum(rng.geometric(0.2, n), 127)
    x[rng.random(n) < 0.5] = 0
    return x.astype(np.uint8).reshape(shape)


def _ragged(lats):
    return torch.from_numpy(np.concatenate([x.reshape(-1) for x in lats])).cuda()


@pytest.fixture(scope="module")
def twelve(codec):
    """(coder, latents, containers, archive bytes) of the 12 mixed shapes, encoded and packed once."""
    rng = np.random.default_rng(31)
    lats = [_skewed(rng, (h, w, LAT_C)) for w, h, _ in SHAPES]
    coder = codec.RaggedLatentCoder([(h, w) for w, h, _ in SHAPES], LAT_C, [(16 * w - i % 5, 16 * h - i % 3) for i, (w, h, _) in enumerate(SHAPES)],
                                    [s for _, _, s in SHAPES])
    coder.encode(_ragged(lats))
    archive = codec.RaggedArchive([coder], tag=77)
    archive.pack()
    b = archive.bytes()
    archive.check()
    return coder, lats, coder.containers(), b


def test_real_coder_archive_is_the_numpy_statement_over_containers(codec, twelve):
    coder, lats, containers, b = twelve
    assert b == ac.make_archive([(c,) for c in containers], 77)
    assert codec.split_archive(b) == [(c,) for c in containers]
    info = codec.archive_info(b)
    assert (info["n_images"], info["n_sections"], info["tag"], info["total_bytes"]) == (len(SHAPES), 1, 77, len(b))
    assert info["image_sizes"] == coder.image_sizes
    assert info["latent_shapes"] == [((h, w, LAT_C),) for w, h, _ in SHAPES]


def test_every_split_container_decodes_alone(codec, twelve):
    _, lats, _, b = twelve
    for i, ((c,), x) in enumerate(zip(codec.split_archive(b), lats)):
        got, info = codec.decode_latent(torch.frombuffer(bytearray(c), dtype=torch.uint8).cuda())
        torch.cuda.synchronize()
        assert int(info.stream_symbols) == SHAPES[i][2]
        assert np.array_equal(got.cpu().numpy(), x), f"image {i}"


def test_unpack_into_a_second_coder_and_decode(codec, twelve):
    coder, lats, _, b = twelve
    other = codec.RaggedLatentCoder(coder.shapes, LAT_C, coder.image_sizes, coder.stream_symbols)
    other.slot_buffer.fill_(SLOT_PATTERN)
    archive = codec.RaggedArchive([other], tag=77)
    valid, = archive.unpack(b)
    back = torch.full((other.latent_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    other.decode(back, valid=valid)
    archive.check()
    other.check()
    assert np.array_equal(back.cpu().numpy(), np.concatenate([x.reshape(-1) for x in lats]))
    assert valid.cpu().tolist() == [[0, s] for s in coder.sizes()]
    # a device tensor is an archive as well, and another tag is not this object's
    assert [v.cpu().tolist() for v in archive.unpack(torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda())] == [[[0, s] for s in coder.sizes()]]
    wrong = codec.RaggedArchive([other], tag=78)
    wrong.unpack(b)
    with pytest.raises(codec._lib.SicnError) as e:
        wrong.check()
    assert e.value.bits == ac.BAD_TAG and e.value.first_bad is None


def test_encoder_error_stays_with_its_image_through_the_archive(codec, lib):
    """An encoder status with an error for image 2 of 5: bit 0, entry 2 of size 0, the others exact; after unpack the decoder
    reports bit 8 for image 2 only and its neighbours decode exactly."""
    shapes = [(2, 3), (3, 3), (1, 2), (3, 5), (2, 7)]
    rng = np.random.default_rng(33)
    lats = [_skewed(rng, (h, w, LAT_C)) for h, w in shapes]
    coder = codec.RaggedLatentCoder(shapes, LAT_C, stream_symbols=2048)
    coder.encode(_ragged(lats))
    containers = coder.containers()
    coder.enc_status[2, 0] = 1
    archive = codec.RaggedArchive([coder], tag=0)
    archive.pack()
    b = archive.bytes()
    assert archive.read_status()[:2] == (ac.PACK_STATUS_ERROR, 2)
    with pytest.raises(lib.SicnError) as e:
        archive.check()
    assert e.value.bits == ac.PACK_STATUS_ERROR and e.value.image == 2
    assert b == ac.make_archive([(b"" if i == 2 else c,) for i, c in enumerate(containers)], 0)
    other = codec.RaggedLatentCoder(shapes, LAT_C, stream_symbols=2048)
    valid, = codec.RaggedArchive([other], tag=0).unpack(b)
    back = torch.full((other.latent_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    other.decode(back, valid=valid)
    torch.cuda.synchronize()
    st = other.dec_status.cpu().numpy().astype(np.int64)
    assert [int(v) & 256 for v in st[:, 0]] == [0, 0, 256, 0, 0] and all(int(v) == 0 for i, v in enumerate(st[:, 0]) if i != 2)
    for i, (v, x) in enumerate(zip(other.views(back), lats)):
        if i != 2:
            assert np.array_equal(v.cpu().numpy(), x), f"image {i}"


def test_net_compress_archive_and_decompress_archive(codec):
    from simple_image_compression_network_amd import api
    sizes = [(17, 9), (48, 48), (100, 36)]                   # (width, height)
    rng = np.random.default_rng(35)
    net = api.RaggedNet(sizes)
    xin = net.pack([torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in sizes])
    containers = net.compress(xin)
    b = net.compress_archive(xin)
    assert [c for c, in codec.split_archive(b)] == containers
    assert b == ac.make_archive([(c,) for c in containers], 0)
    want = net.decompress(containers)
    got = net.decompress_archive(b)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ---- 10: the hyperprior codec -----------------------------------------------------------------------------------------------------------
HYPER_SIZES = [(17, 33), (100, 36), (33, 1)]                # (width, height), three of tests/test_ragged_hyper_gpu.py
SEED = 7


@pytest.fixture(scope="module")
def hyper(lib):
    from simple_image_compression_network_amd import hyperprior
    codec = hyperprior.RaggedHyperpriorCodec(HYPER_SIZES, seed=SEED)
    rng = np.random.default_rng(37)
    codec.encode(codec.main.pack([torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in HYPER_SIZES]))
    out = codec.decode()
    codec.check()
    return hyperprior, codec, codec.containers(), codec.archive(), out.clone()


def test_hyperprior_archive_splits_to_its_containers(codec, lib, hyper):
    _, hc, containers, b, _ = hyper
    tag = int(lib.lib().sicn_gdn_spec_version())
    assert tag != 0 and hc.archive_tag == tag
    assert codec.split_archive(b) == containers
    assert b == ac.make_archive(containers, tag)
    info = codec.archive_info(b)
    assert (info["n_images"], info["n_sections"], info["tag"]) == (len(HYPER_SIZES), 2, tag) and info["image_sizes"] == HYPER_SIZES


def test_a_second_codec_from_the_archive_reconstructs_the_same_bytes(hyper):
    hyperprior, hc, _, b, out = hyper
    other = hyperprior.RaggedHyperpriorCodec.from_archive(b, seed=SEED)
    assert other.sizes == HYPER_SIZES and other.use_gdn and other.z_coder.stream_symbols == hc.z_coder.stream_symbols
    got = other.decode(archive=b)
    other.check()
    torch.cuda.synchronize()
    assert torch.equal(got, out) and torch.equal(other.y_hat, hc.y)


def test_a_codec_without_gdn_refuses_a_gdn_archive(lib, hyper):
    hyperprior, _, _, b, _ = hyper
    plain = hyperprior.RaggedHyperpriorCodec(HYPER_SIZES, seed=SEED, use_gdn=False)
    assert plain.archive_tag == 0
    plain.decode(archive=b)
    with pytest.raises(lib.SicnError) as e:
        plain.check()
    assert e.value.bits == ac.BAD_TAG
    torch.cuda.synchronize()
    assert [int(v) & 256 for v in plain.z_coder.dec_status[:, 0].cpu()] == [256] * len(HYPER_SIZES)      # every slot is empty for the decoders
    assert [int(v) & 256 for v in plain.y_coder.dec_status[:, 0].cpu()] == [256] * len(HYPER_SIZES)


def test_a_damaged_y_container_in_a_valid_archive_is_reported_for_its_image_only(codec, lib, hyper):
    hyperprior, hc, containers, b, _ = hyper
    bad = 1
    info, sizes, offsets = codec._parse_archive(b)
    broken = bytearray(b)
    broken[offsets[bad * 2 + 1] + sizes[bad * 2 + 1] - 3] ^= 0x04
    other = hyperprior.RaggedHyperpriorCodec.from_archive(bytes(broken), seed=SEED)
    other.decode(archive=bytes(broken))
    with pytest.raises(lib.SicnError) as e:
        other.check()
    assert e.value.image == bad and f"image {bad}" in str(e.value)
    assert other._archive.read_status()[0] == 0                 # the archive itself is sound
    for i, (a, ref) in enumerate(zip(other.main.views(3, other.y_hat), hc.main.views(3, hc.y))):
        if i != bad:
            assert torch.equal(a, ref), f"image {i}"


# ---- 11: capture --------------------------------------------------------------------------------------------------------------------------
def test_encode_and_pack_are_captured_in_one_graph(codec):
    shapes = [(1, 1), (2, 3), (3, 5), (12, 16), (2, 7)]
    rng = np.random.default_rng(39)
    first, fresh = ([_skewed(rng, (h, w, LAT_C)) for h, w in shapes] for _ in range(2))
    coder = codec.RaggedLatentCoder(shapes, LAT_C, stream_symbols=2048)
    archive = codec.RaggedArchive([coder], tag=4)
    coder.encode(_ragged(fresh))                             # eager, on the latents the replay will see (also the warm-up)
    archive.pack()
    want = archive.bytes()
    archive.check()
    assert codec.split_archive(want) == [(c,) for c in coder.containers()]
    x = _ragged(first)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):           # one stream, no parallel branches
            coder.encode(x)
            archive.pack()
    x.copy_(_ragged(fresh))
    coder.slot_buffer.zero_()
    coder.enc_status.zero_()
    archive.buffer.fill_(OUT_PATTERN)
    archive.status.fill_(-1)
    graph.replay()
    assert archive.bytes() == want
    archive.check()
