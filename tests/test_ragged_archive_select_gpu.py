"""GPU checks of random access into a ragged archive (include/sicn_ragged_archive_select.h, k_archive_parse_select in
csrc/k_ragged_archive.hip; run with -m gpu on an MI355X): the containers of a SELECTION of an archive's images unpacked into an
object made for those images, with two launches.  Everything is byte equality: against the numpy statement of the format in
tests/archive_cases.py, against sicn_ragged_archive_unpack_async of the whole archive (the identity selection) and against
sicn_ragged_archive_unpack_async of sicn_ragged_archive_subset's archive (any selection).  Most cases drive the C entry points with
numpy-made archives of random bytes, slot buffers and `valid` arrays pre-filled with a guard pattern; the last ones go through the real
coders, the net and the hyperprior codec."""
import ctypes

import numpy as np
import pytest

import archive_cases as ac

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL, ENOSPC = -22, -28
SLOT_PATTERN = 0x5A
BAD_SELECTION = 256                                         # status bit 8
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


def _upload(b: bytes, odd=0):
    """The archive in device memory, beginning `odd` bytes into its allocation."""
    base = torch.empty(len(b) + 32, dtype=torch.uint8, device="cuda")
    view = base[odd:odd + len(b)]
    if b:
        view.copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return view


def _index(sel):
    return torch.from_numpy(np.asarray(sel, dtype=np.uint32).view(np.int32).copy()).cuda()


class Slots:
    """An archive object over k sections of n slots of caps[j][s] bytes, back to back at multiples of 16 (plus a gap here and there),
    every slot byte and every `valid` word holding a guard pattern before each call.  `odd`: every slot buffer begins `odd` bytes
    into its allocation."""

    def __init__(self, lib, caps, odd=0):
        self.L = lib.lib()
        self.caps = np.asarray(caps, dtype=np.int64)
        self.n, self.k = self.caps.shape
        self.off, self.slots = [], []
        for s in range(self.k):
            at, offs = 0, []
            for j in range(self.n):
                offs.append(at)
                at += ac.a16(self.caps[j, s]) + 16 * ((j + s) % 3 == 0)
            self.off.append(offs)
            base = torch.empty(max(at, 16) + 16, dtype=torch.uint8, device="cuda")
            self.slots.append(base[odd:odd + max(at, 16)])
        self._tables = [(ctypes.c_uint64 * self.n)(*offs) for offs in self.off], \
                       [(ctypes.c_uint64 * self.n)(*[int(v) for v in self.caps[:, s]]) for s in range(self.k)]
        pp = U64P * self.k
        self.h = ctypes.c_void_p()
        rc = self.L.sicn_ragged_archive_create(self.n, self.k, pp(*[ctypes.cast(a, U64P) for a in self._tables[0]]),
                                               pp(*[ctypes.cast(a, U64P) for a in self._tables[1]]), ctypes.byref(self.h))
        assert rc == 0, rc
        self.ws_bytes = int(self.L.sicn_ragged_archive_workspace_bytes(self.h))
        self.ws = torch.empty(max(self.ws_bytes, 16), dtype=torch.uint8, device="cuda")
        self.st = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.valid = [torch.empty((self.n, 2), dtype=torch.int32, device="cuda") for _ in range(self.k)]

    def __del__(self):
        if getattr(self, "h", None):
            self.L.sicn_ragged_archive_free(self.h)
            self.h = None

    def ptrs(self, tensors):
        return (ctypes.c_void_p * self.k)(*[t.data_ptr() for t in tensors])

    def guard(self):
        for t in self.slots:
            t.fill_(SLOT_PATTERN)
        for v in self.valid:
            v.fill_(-1)
        self.st.fill_(-7)

    def unpack(self, src, n_in, tag):
        self.guard()
        return self.L.sicn_ragged_archive_unpack_async(self.h, _vp(src), n_in, tag, self.ptrs(self.slots), self.ptrs(self.valid), _vp(self.st),
                                                       _vp(self.ws), self.ws.numel(), None)

    def select(self, src, n_in, tag, index, ws_bytes=None):
        self.guard()
        return self.L.sicn_ragged_archive_unpack_select_async(
            self.h, _vp(src), n_in, tag, _vp(index) if index is not None else None, self.ptrs(self.slots), self.ptrs(self.valid), _vp(self.st),
            _vp(self.ws), self.ws.numel() if ws_bytes is None else ws_bytes, None)

    def state(self):
        """(slot buffers, valid arrays, (error, first_bad, bytes)) as the last call left them."""
        torch.cuda.synchronize()
        e, bad, lo, hi = (int(v) & 0xFFFFFFFF for v in self.st.cpu().tolist())
        return [t.cpu().numpy() for t in self.slots], [v.cpu().numpy().astype(np.int64) & 0xFFFFFFFF for v in self.valid], (e, bad, lo | hi << 32)

    def expected(self, containers):
        """What the slot buffers and valid arrays must hold after containers[j][s] went to slot j of section s."""
        slots, valid = [], []
        for s in range(self.k):
            want = np.full(self.slots[s].numel(), SLOT_PATTERN, np.uint8)
            for j in range(self.n):
                c = np.frombuffer(containers[j][s], dtype=np.uint8)
                want[self.off[s][j]:self.off[s][j] + c.size] = c
            slots.append(want)
            valid.append(np.array([[0, len(containers[j][s])] for j in range(self.n)], dtype=np.int64))
        return slots, valid


def _same(got, want, what):
    for s, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}, section {s}: first difference at {int(np.flatnonzero(a.reshape(-1) != b.reshape(-1))[0])}"


def _caps_for(sizes, sel):
    """Capacities of the object for the selection: here the container's own size (a full slot), there some bytes more."""
    sizes = np.asarray(sizes, dtype=np.int64)
    return np.array([[sizes[i, s] + (0 if (j + s) % 3 == 0 else 1 + 37 * ((j + s) % 4)) for s in range(sizes.shape[1])] for j, i in enumerate(sel)])


def _check_select(lib, sizes, sel, seed, tag=0x1234ABCD, odd_slots=0, odd_archive=0):
    """unpack_select(A, sel) leaves what the numpy statement says AND what unpack(subset(A, sel)) leaves: slot buffers with their guard
    bytes, valid arrays and status.error; status.bytes is len(A) here and the subset's length there."""
    sizes = np.asarray(sizes, dtype=np.int64)
    n_all, k = sizes.shape
    containers = ac.sample_containers(n_all, k, seed=seed, sizes=sizes.tolist())
    a = ac.make_archive(containers, tag)
    obj = Slots(lib, _caps_for(sizes, sel), odd=odd_slots)
    src = _upload(a, odd_archive)
    assert src.data_ptr() % 16 == odd_archive % 16 and all(t.data_ptr() % 16 == odd_slots % 16 for t in obj.slots)
    assert obj.select(src, len(a), tag, _index(sel)) == 0
    slots, valid, status = obj.state()
    assert status == (0, ac.NO_ENTRY, len(a))
    want_slots, want_valid = obj.expected([containers[i] for i in sel])
    _same(slots, want_slots, "select against numpy: slot bytes")
    _same(valid, want_valid, "select against numpy: valid")
    from simple_image_compression_network_amd import codec
    sub = codec.subset_archive(a, sel)
    assert sub == ac.make_archive([containers[i] for i in sel], tag)
    assert obj.unpack(_upload(sub, odd_archive), len(sub), tag) == 0
    slots2, valid2, status2 = obj.state()
    assert status2 == (0, ac.NO_ENTRY, len(sub))
    _same(slots, slots2, "select against unpack of the subset: slot bytes")
    _same(valid, valid2, "select against unpack of the subset: valid")
    return obj


def _edge_sizes(lib, k):
    c = _chunk(lib)
    edge = [0, 1, 15, 16, 17, c - 1, c, c + 1, 2 * c + 5, 3 * c + 7]
    return np.array([[edge[(i + 3 * s) % len(edge)] for s in range(k)] for i in range(len(edge))])


# ---- identity: every image selected -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 4])
def test_identity_selection_is_unpack(lib, k):
    sizes = _edge_sizes(lib, k)
    n = len(sizes)
    containers = ac.sample_containers(n, k, seed=60 + k, sizes=sizes.tolist())
    a = ac.make_archive(containers, 5)
    obj = Slots(lib, _caps_for(sizes, range(n)))
    src = _upload(a)
    assert obj.unpack(src, len(a), 5) == 0
    slots, valid, status = obj.state()
    assert status == (0, ac.NO_ENTRY, len(a))
    assert obj.select(src, len(a), 5, _index(range(n))) == 0
    slots2, valid2, status2 = obj.state()
    assert status2 == status
    _same(slots2, slots, "slot bytes")
    _same(valid2, valid, "valid")
    _same(slots2, obj.expected(containers)[0], "slot bytes against numpy")


# ---- select == unpack of the subset -----------------------------------------------------------------------------------------------------
def _random_sizes(n, k, seed):
    """0 .. 40 bytes, a third of them empty: empty containers fall inside and outside every selection."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 41, (n, k))
    sizes[rng.random((n, k)) < 0.33] = 0
    return sizes


def _pass_cases():
    cases = []
    for k in (1, 2):
        edge = 256 // k                                    # the first image of the second pass of 256 entries
        for n in (edge - 1, edge, edge + 1):                 # 255, 256, 257 entries at k = 1; 254, 256, 258 at k = 2
            sel = sorted({0, edge - 2, edge - 1, edge} & set(range(n)))     # the last image of a pass and the first of the next
            cases.append(pytest.param(n, k, sel, id=f"N{n}_k{k}_straddle"))
        cases.append(pytest.param(5000, k, [0, 2499, 4999], id=f"N5000_k{k}_three"))
        cases.append(pytest.param(600, k, [599], id=f"N600_k{k}_last_only"))
        cases.append(pytest.param(600, k, list(range(1, 600, 2)), id=f"N600_k{k}_300_of_600"))
        cases.append(pytest.param(600, k, list(range(150, 450)), id=f"N600_k{k}_300_in_a_row"))
    # an image whose sections lie in two passes (k = 3: image 85 is entries 255, 256, 257), and four sections
    cases.append(pytest.param(100, 3, [84, 85, 86], id="N100_k3_image_across_passes"))
    cases.append(pytest.param(100, 3, [85], id="N100_k3_only_that_image"))
    cases.append(pytest.param(130, 4, [0, 63, 64, 65, 129], id="N130_k4_straddle"))
    return cases


@pytest.mark.parametrize("n_all,k,sel", _pass_cases())
def test_select_equals_unpack_of_the_subset(lib, n_all, k, sel):
    _check_select(lib, _random_sizes(n_all, k, seed=n_all + k), sel, seed=n_all * 7 + k, tag=n_all)


@pytest.mark.parametrize("k", [1, 2])
def test_chunk_and_vector_edges_selected_and_not(lib, k):
    """Containers of exactly a chunk, a chunk +- 1, 15 / 16 / 17 bytes and none, selected and passed over."""
    sizes = _edge_sizes(lib, k)
    n = len(sizes)
    for sel in (list(range(n)), [2, 3, 4, 5, 6, 7], [0, 9], [5], [1, 3, 6, 8]):
        _check_select(lib, sizes, sel, seed=70 + k)


@pytest.mark.parametrize("k,odd_slots,odd_archive", [(1, 1, 3), (2, 3, 1)])
def test_byte_path_gives_the_same_bytes(lib, k, odd_slots, odd_archive):
    """The archive and the slot buffers as views at odd offsets: no 16-byte vector is possible, the index is read bytewise, and the
    bytes are the numpy statement's all the same."""
    sizes = _edge_sizes(lib, k)
    _check_select(lib, sizes, [1, 4, 5, 6, 9], seed=80 + k, odd_slots=odd_slots, odd_archive=odd_archive)
    _check_select(lib, sizes, [1, 4, 5, 6, 9], seed=80 + k, odd_slots=0, odd_archive=odd_archive)
    _check_select(lib, sizes, [1, 4, 5, 6, 9], seed=80 + k, odd_slots=odd_slots, odd_archive=0)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
REFUSAL_SIZES = [[17, 40], [0, 16], [1, 33], [5, 0]]
REFUSAL_SEL = [1, 3]


def _refusal_object(lib, sel=REFUSAL_SEL, extra=16):
    containers = ac.sample_containers(4, 2, seed=6, sizes=REFUSAL_SIZES)
    caps = np.array([[ac.a16(REFUSAL_SIZES[i][s]) + extra for s in range(2)] for i in sel])
    return Slots(lib, caps), containers, ac.make_archive(containers, 9)


def _assert_refused(obj, archive, n_in, tag, sel, bit, want_bad=ac.NO_ENTRY, want_bytes=None):
    src = _upload(archive)
    assert obj.select(src, n_in, tag, _index(sel)) == 0
    slots, valid, (e, bad, nbytes) = obj.state()
    assert e & bit and not e & ~0x1F8, f"status {e:#x}, expected bit {bit:#x}"
    assert bad == want_bad
    if want_bytes is not None:
        assert nbytes == want_bytes
    for s in range(obj.k):
        assert (valid[s][:, 0] == e).all() and (valid[s][:, 1] == 0).all(), "every valid entry of a refused archive is {error, 0}"
        assert (slots[s] == SLOT_PATTERN).all(), "a refused archive wrote a slot byte"
    return e


def test_every_refusal_is_clean(lib):
    obj, containers, good = _refusal_object(lib)
    n_all, k = 4, 2
    assert obj.select(_upload(good), len(good), 9, _index(REFUSAL_SEL)) == 0
    _same(obj.state()[0], obj.expected([containers[i] for i in REFUSAL_SEL])[0], "the good archive")
    # bit 8: an index == N, equal neighbours, descending — the archive itself is sound, its size is reported
    for sel in ([1, n_all], [3, 3], [3, 1], [0xFFFFFFFF, 1]):
        assert _assert_refused(obj, good, len(good), 9, sel, BAD_SELECTION, want_bytes=len(good)) == BAD_SELECTION, sel
    # bit 4: more images asked for than the archive holds (an archive of ONE image for this object of two); another n_sections
    one = ac.make_archive(containers[:1], 9)
    assert _assert_refused(obj, one, len(one), 9, [0, 1], ac.BAD_COUNTS, want_bytes=0) == ac.BAD_COUNTS
    other_k = ac.make_archive([c + (b"",) for c in containers], 9)
    assert _assert_refused(obj, other_k, len(other_k), 9, REFUSAL_SEL, ac.BAD_COUNTS, want_bytes=0) == ac.BAD_COUNTS
    # bit 5: the tag
    assert _assert_refused(obj, good, len(good), 10, REFUSAL_SEL, ac.BAD_TAG, want_bytes=len(good)) == ac.BAD_TAG
    # bit 6: a SELECTED entry one byte over its slot, the archive consistent: the entry is named in the object's numbering
    j, s = 1, 0                                             # image 3, section 0 -> object entry 1 * 2 + 0
    cap = int(obj.caps[j, s])
    over = ac.make_archive([tuple(b"\x01" * (cap + 1) if (i, t) == (REFUSAL_SEL[j], s) else c for t, c in enumerate(cs)) for i, cs in enumerate(containers)], 9)
    assert _assert_refused(obj, over, len(over), 9, REFUSAL_SEL, ac.BAD_SIZE, want_bad=j * k + s, want_bytes=len(over)) == ac.BAD_SIZE
    # bit 7: ONE UNSELECTED entry's size patched so that the sum breaks (image 2, section 1: 33 -> 49)
    assert _assert_refused(obj, ac.patched(good, 32 + 4 * 5, "<I", 49), len(good), 9, REFUSAL_SEL, ac.BAD_TOTAL) == ac.BAD_TOTAL
    # bit 7: in_bytes one short of total_bytes
    assert _assert_refused(obj, good, len(good) - 1, 9, REFUSAL_SEL, ac.BAD_TOTAL) == ac.BAD_TOTAL
    # bit 3: each header patch of the hostile archives, and nothing behind such a header is looked at; a buffer shorter than a header
    for name, bad, bit in ac.hostile(good, n_all, k):
        if bit == ac.BAD_HEADER:
            assert _assert_refused(obj, bad, len(bad), 9, REFUSAL_SEL, ac.BAD_HEADER, want_bytes=0) == ac.BAD_HEADER, name
    assert _assert_refused(obj, good[:31], 31, 9, REFUSAL_SEL, ac.BAD_HEADER, want_bytes=0) == ac.BAD_HEADER
    # ... and the index's padding (3 x 2 entries: 8 bytes of it)
    padded = ac.make_archive(containers[:3], 9)
    pobj = Slots(lib, np.array([[64, 64]]))
    assert pobj.select(_upload(padded), len(padded), 9, _index([1])) == 0 and pobj.state()[2][0] == 0
    assert _assert_refused(pobj, ac.patched(padded, 32 + 28, "<B", 1), len(padded), 9, [1], ac.BAD_HEADER) & ac.BAD_HEADER
    # the object is as good as before
    assert obj.select(_upload(good), len(good), 9, _index(REFUSAL_SEL)) == 0
    slots, valid, status = obj.state()
    assert status == (0, ac.NO_ENTRY, len(good))
    _same(slots, obj.expected([containers[i] for i in REFUSAL_SEL])[0], "after the refusals")


def test_an_unselected_entry_larger_than_every_slot_is_no_error(lib):
    c = _chunk(lib)
    sizes = [[17, 40], [0, 16], [3 * c + 7, 33], [5, 0], [9, 2 * c]]
    obj = _check_select(lib, sizes, [1, 3], seed=91)
    assert int(obj.caps.max()) < 2 * c


def test_argument_checks_with_an_object(lib):
    """A short workspace gives SICN_ENOSPC, a NULL or misaligned index SICN_EINVAL, and nothing is enqueued: neither the status nor
    a slot byte nor a valid word changes."""
    obj, containers, good = _refusal_object(lib)
    src = _upload(good)
    index = _index([0] + REFUSAL_SEL)
    assert obj.select(src, len(good), 9, index[1:], ws_bytes=obj.ws_bytes - 1) == ENOSPC
    assert obj.select(src, len(good), 9, index[1:], ws_bytes=0) == ENOSPC
    assert obj.select(src, len(good), 9, None) == EINVAL
    odd = index.view(torch.uint8)[2:10]
    assert odd.data_ptr() % 4 == 2
    assert obj.select(src, len(good), 9, odd) == EINVAL
    slots, valid, _ = obj.state()
    assert (obj.st.cpu().numpy() == -7).all()
    assert all((t == SLOT_PATTERN).all() for t in slots) and all((v == 0xFFFFFFFF).all() for v in valid)
    assert obj.select(src, len(good), 9, index[1:], ws_bytes=obj.ws_bytes) == 0      # exactly enough is enough; 4-byte alignment is
    assert obj.state()[2] == (0, ac.NO_ENTRY, len(good))


# ---- the real coders --------------------------------------------------------------------------------------------------------------------
NET_SIZES = [(17, 9), (48, 48), (100, 36), (16, 16), (33, 1), (1, 1), (64, 20), (20, 64), (48, 48), (31, 17), (5, 50), (80, 24)]   # (width, height)


@pytest.fixture(scope="module")
def twelve(codec):
    """(the net of all twelve images, their archive, the full reconstruction's per-image arrays), made once."""
    from simple_image_compression_network_amd import api
    rng = np.random.default_rng(41)
    net = api.RaggedNet(NET_SIZES)
    xin = net.pack([torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in NET_SIZES])
    b = net.compress_archive(xin)
    out = net.decompress_archive(b)
    torch.cuda.synchronize()
    return api, net, b, [v.clone() for v in net.views(7, out)]


@pytest.mark.parametrize("sel", [[0], [11], [1, 4, 5, 11]], ids=["first", "last", "four"])
def test_net_decompresses_a_selection(codec, twelve, sel):
    api, net, b, full = twelve
    small = api.RaggedNet.from_archive(b, images=sel, shared_weights=net.weights)
    assert small.sizes == [NET_SIZES[i] for i in sel]
    out = small.decompress_archive(b, images=sel)
    torch.cuda.synchronize()
    for j, i in enumerate(sel):
        assert torch.equal(small.views(7, out)[j], full[i]), f"image {i}"
    sub = codec.subset_archive(b, sel)
    assert codec.split_archive(sub) == [codec.split_archive(b)[i] for i in sel]
    out2 = small.decompress_archive(sub).clone()
    torch.cuda.synchronize()
    assert torch.equal(out2, small.decompress_archive(b, images=sel))


def test_net_refuses_a_selection_that_is_none_before_any_launch(twelve):
    api, net, b, _ = twelve
    small = api.RaggedNet.from_archive(b, images=[1, 4], shared_weights=net.weights)
    for bad in ([4, 1], [1, 1], [1], [1, 4, 5], [1, 12], [-1, 4]):
        with pytest.raises(ValueError):
            small.decompress_archive(b, images=bad)
    with pytest.raises(ValueError):
        small.decompress_archive(b, images=[1, 5])           # a sound selection of other sizes than this net's
    with pytest.raises(ValueError):
        api.RaggedNet.from_archive(b, images=[5, 4])
    assert api.RaggedNet.from_archive(b, shared_weights=net.weights).sizes == NET_SIZES


def test_archive_object_reports_bit_8(codec, twelve):
    """A device tensor of indices is taken as it lies: the device finds that it is no selection, and check() says so."""
    api, net, b, _ = twelve
    small = api.RaggedNet.from_archive(b, images=[1, 4], shared_weights=net.weights)
    coder = small.latent_coder(16384)
    archive = codec.RaggedArchive([coder], tag=0)
    with pytest.raises(ValueError):
        archive.unpack(b, images=[4, 1])
    with pytest.raises(ValueError):
        archive.unpack(b, images=[1, 4, 5])
    archive.unpack(b, images=torch.tensor([4, 1], dtype=torch.int32, device="cuda"))
    with pytest.raises(codec._lib.SicnError) as e:
        archive.check()
    assert e.value.bits == BAD_SELECTION and e.value.first_bad is None
    valid, = archive.unpack(b, images=[1, 4])
    archive.check()
    sizes = [len(c) for c, in codec.split_archive(b)]
    assert valid.cpu().tolist() == [[0, sizes[1]], [0, sizes[4]]]


# ---- the hyperprior codec ---------------------------------------------------------------------------------------------------------------
HYPER_SIZES = [(17, 33), (100, 36), (33, 1)]                # (width, height), those of tests/test_ragged_archive_gpu.py
HYPER_SEL = [0, 2]
SEED = 7


@pytest.fixture(scope="module")
def hyper(lib):
    from simple_image_compression_network_amd import hyperprior
    full = hyperprior.RaggedHyperpriorCodec(HYPER_SIZES, seed=SEED)
    rng = np.random.default_rng(43)
    full.encode(full.main.pack([torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in HYPER_SIZES]))
    b = full.archive()
    out = full.decode(archive=b)
    full.check()
    torch.cuda.synchronize()
    return hyperprior, b, [v.clone() for v in full.main.views(7, out)]


def test_hyperprior_decodes_a_selection(hyper):
    hyperprior, b, full = hyper
    other = hyperprior.RaggedHyperpriorCodec.from_archive(b, seed=SEED, images=HYPER_SEL)
    assert other.sizes == [HYPER_SIZES[i] for i in HYPER_SEL] and other.use_gdn
    out = other.decode(archive=b, images=HYPER_SEL)
    other.check()
    torch.cuda.synchronize()
    for j, i in enumerate(HYPER_SEL):
        assert torch.equal(other.main.views(7, out)[j], full[i]), f"image {i}"
    with pytest.raises(ValueError):
        other.decode(archive=b, images=[2, 0])
    with pytest.raises(ValueError):
        other.decode(images=HYPER_SEL)


def test_a_codec_without_gdn_refuses_a_gdn_archive_through_the_select_path(lib, hyper):
    hyperprior, b, _ = hyper
    plain = hyperprior.RaggedHyperpriorCodec([HYPER_SIZES[i] for i in HYPER_SEL], seed=SEED, use_gdn=False)
    assert plain.archive_tag == 0
    plain.decode(archive=b, images=HYPER_SEL)
    with pytest.raises(lib.SicnError) as e:
        plain.check()
    assert e.value.bits == ac.BAD_TAG
    torch.cuda.synchronize()
    assert [int(v) & 256 for v in plain.z_coder.dec_status[:, 0].cpu()] == [256] * len(HYPER_SEL)      # every slot is empty for the decoders
    assert [int(v) & 256 for v in plain.y_coder.dec_status[:, 0].cpu()] == [256] * len(HYPER_SEL)


# ---- capture ----------------------------------------------------------------------------------------------------------------------------
def test_select_unpack_and_decode_are_captured_in_one_graph(codec):
    """Two pairs of equal latent shapes in one archive; the graph unpacks `index` and decodes.  The index array is rewritten between
    the replays: the second one gives the other pair's bytes."""
    lat_c = 192
    shapes = [(2, 3), (3, 5), (2, 3), (3, 5)]
    rng = np.random.default_rng(45)
    lats = []
    for h, w in shapes:
        x = np.minimum(rng.geometric(0.2, h * w * lat_c), 127)
        x[rng.random(x.size) < 0.5] = 0
        lats.append(x.astype(np.uint8))
    enc = codec.RaggedLatentCoder(shapes, lat_c, stream_symbols=2048)
    enc.encode(torch.from_numpy(np.concatenate(lats)).cuda())
    packer = codec.RaggedArchive([enc], tag=4)
    packer.pack()
    resident = torch.frombuffer(bytearray(packer.bytes()), dtype=torch.uint8).cuda()       # the archive stays on the device
    packer.check()
    dec = codec.RaggedLatentCoder(shapes[:2], lat_c, stream_symbols=2048)
    archive = codec.RaggedArchive([dec], tag=4)
    index = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    back = torch.empty(dec.latent_bytes, dtype=torch.uint8, device="cuda")

    def run():
        valid, = archive.unpack(resident, images=index)
        dec.decode(back, valid=valid)

    run()                                                    # eager: the warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):           # one stream, no parallel branches
            run()
    for sel in ([0, 1], [2, 3], [0, 3]):
        index.copy_(torch.tensor(sel, dtype=torch.int32))
        back.fill_(0xEE)
        dec.slot_buffer.fill_(SLOT_PATTERN)
        graph.replay()
        archive.check()
        dec.check()
        assert np.array_equal(back.cpu().numpy(), np.concatenate([lats[i] for i in sel])), sel
