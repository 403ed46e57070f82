"""What tests/test_large_tensors_gpu.py rests on, without a GPU (tests/large_tensor_cases.py).
The checker: a result of 2 GiB is compared band by band and window by window, so `valid`, `band_plan` and `window` are held to the C
oracle at 70 x 50: the oracle on a whole image is the oracle's bands stitched, for 1, 2, 3 and 7 bands and odd heights; a wrong byte
planted in a row at a band seam is seen; a window's valid part is the whole image's.
The shapes: every byte count relative to L = 2^31 and to 2^32 is asserted here by arithmetic, so a typo in a shape cannot turn a limit
case into an ordinary one.  The ragged layout (sicn_ragged_layout, host only) gives the offsets past 2^32 as Python integers and refuses
an image of exactly L bytes on either side of a layer."""
import ctypes

import numpy as np
import pytest

import large_tensor_cases as lt
from simple_image_compression_network_amd import _lib
from simple_image_compression_network_amd.config import CLayerDesc

SEED = 31
CHAIN_KINDS = [("conv",), ("deconv",), ("l0", "conv"), ("deconv", "rgb"), ("conv", "conv")]      # the five chain kinds of the GPU file
W = 70


@pytest.fixture(scope="module")
def whole():
    """(input, oracle output) per (kinds, height), computed once"""
    cache = {}

    def get(kinds, h):
        if (kinds, h) not in cache:
            cin = lt.KINDS[kinds[0]][0]
            x = np.random.default_rng([SEED, h, cin]).integers(0, 256, (h, W, cin), dtype=np.uint8)
            y = lt.oracle_chain(kinds, lt.chain_weights(kinds, SEED), x)
            x.setflags(write=False)
            y.setflags(write=False)
            cache[(kinds, h)] = (x, y)
        return cache[(kinds, h)]
    return get


@pytest.mark.parametrize("h", [50, 51, 53])
@pytest.mark.parametrize("kinds", CHAIN_KINDS, ids="-".join)
def test_oracle_bands_stitched_are_the_oracle_on_the_whole_image(whole, kinds, h):
    x, y = whole(kinds, h)
    wb = lt.chain_weights(kinds, SEED)
    for n_bands in (1, 2, 3, 7):
        plan = lt.band_plan(kinds, h, n_bands)
        assert [p for _, _, p, _, _ in plan] + [plan[-1][3]] == sorted({y.shape[0] * k // n_bands for k in range(n_bands + 1)})
        assert all(a % lt.alignment(kinds) == 0 and 0 <= a < b <= h for a, b, _, _, _ in plan)
        if n_bands > 1:
            assert any(b < h for _, b, _, _, _ in plan) and any(a > 0 for a, _, _, _, _ in plan)     # real cuts, not the image each time
        got = lt.stitched(kinds, n_bands, lambda band: lt.oracle_chain(kinds, wb, band), x)
        assert lt.first_difference(got, y) is None, (kinds, h, n_bands, lt.first_difference(got, y))


@pytest.mark.parametrize("kinds", CHAIN_KINDS, ids="-".join)
def test_a_band_one_row_larger_than_valid_says_is_wrong(whole, kinds):
    """the margins are not generous: a row just outside what `valid` gives differs from the whole image's (random weights and pixels)"""
    h = 51
    x, y = whole(kinds, h)
    wb = lt.chain_weights(kinds, SEED)
    al = lt.alignment(kinds)
    a, b = 3 * al, 3 * al + 28
    lo, hi, off = lt.valid(kinds, a, b, h)
    band = lt.oracle_chain(kinds, wb, np.ascontiguousarray(x[a:b]))
    assert 0 < lo < hi < band.shape[0]
    assert np.array_equal(band[lo:hi], y[off + lo:off + hi])
    assert not np.array_equal(band[lo - 1], y[off + lo - 1]) and not np.array_equal(band[hi], y[off + hi])


@pytest.mark.parametrize("kinds", CHAIN_KINDS, ids="-".join)
def test_a_wrong_byte_in_a_row_at_a_band_seam_is_seen(whole, kinds):
    h = 53
    x, y = whole(kinds, h)
    wb = lt.chain_weights(kinds, SEED)
    runs = {}

    def run_band(a, b):
        if (a, b) not in runs:
            runs[(a, b)] = lt.oracle_chain(kinds, wb, np.ascontiguousarray(x[a:b]))
        return runs[(a, b)]
    for n_bands in (3, 7):
        lt.check_bands(kinds, h, n_bands, y, run_band, "clean")
        seams = sorted({r for _, _, p, q, _ in lt.band_plan(kinds, h, n_bands) for r in (p, q - 1)})
        assert seams[0] == 0 and seams[-1] == y.shape[0] - 1
        for row in seams:
            bad = y.copy()
            xx, c = (row * 7) % y.shape[1], (row * 5) % y.shape[2]
            bad[row, xx, c] ^= 1
            with pytest.raises(AssertionError, match=rf"\(row {row}, x {xx}, channel {c}\)"):
                lt.check_bands(kinds, h, n_bands, bad, run_band, "planted")


@pytest.mark.parametrize("kinds", CHAIN_KINDS, ids="-".join)
def test_windows_are_the_whole_image_where_they_say_so(whole, kinds):
    h = 51
    x, y = whole(kinds, h)
    wb = lt.chain_weights(kinds, SEED)
    for oy, ox in lt.window_positions(kinds, W, h, SEED, last_rows=True):
        y0, y1, ylo, yhi, yoff = lt.window(kinds, h, oy, lt.WINDOW_H)
        x0, x1, xlo, xhi, xoff = lt.window(kinds, W, ox, lt.WINDOW_W)
        assert y1 - y0 <= lt.WINDOW_H and x1 - x0 <= lt.WINDOW_W
        ref = lt.oracle_chain(kinds, wb, np.ascontiguousarray(x[y0:y1, x0:x1]))
        assert np.array_equal(ref[ylo:yhi, xlo:xhi], y[yoff + ylo:yoff + yhi, xoff + xlo:xoff + xhi]), (oy, ox)


# ---- the shapes, by arithmetic -------------------------------------------------------------------------------------------------------
def test_single_images_meet_the_limit_on_the_side_they_name_and_pass_it_one_row_higher():
    assert lt.L == 2 ** 31 == 2147483648
    for name, (kinds, w, h, _, _, _, side, below) in lt.SINGLE.items():
        i, o = lt.tensor_bytes(kinds, w, h)
        assert max(i, o) == (i if side == "in" else o) == lt.L - below, (name, i, o)
        assert below in (524288, 1048576)                           # one row of the tensor at the limit
        i1, o1 = lt.tensor_bytes(kinds, w, h + 1)
        assert max(i1, o1) == lt.L, (name, i1, o1)                  # exactly L: the first refused value
        assert o >= lt.NT_MIN_BYTES or name == "conv16-generic"     # they store non-temporal where their kernel can (the generic one cannot)
    assert lt.tensor_bytes(("conv",), 4096, 4095) == [2146959360, 2048 * 2048 * 128]
    assert lt.tensor_bytes(("deconv",), 2048, 2047)[1] == 4096 * 4094 * 128 == lt.L - 1048576
    assert lt.tensor_bytes(("l0",), 8192, 8190)[1] == 4096 * 4095 * 128
    assert lt.tensor_bytes(("conv64",), 8192, 4095)[0] == 8192 * 4095 * 64 == lt.L - 524288


def test_chains_put_the_intermediate_tensor_at_the_limit():
    for name, (kinds, w, h, _, _) in lt.CHAINS.items():
        b = lt.tensor_bytes(kinds, w, h)
        assert len(b) == 3 and max(b) == b[1], (name, b)
    assert lt.tensor_bytes(*lt.CHAINS["l0-conv"][:3])[1] == lt.L - 524288
    assert lt.tensor_bytes(*lt.CHAINS["deconv-l7"][:3])[1] == lt.L - 1048576
    # the power-of-two offsets of the windows lie inside the outputs that have them
    assert lt.tensor_bytes(("conv",), 4096, 4095)[1] == 2 ** 29 and lt.tensor_bytes(("deconv",), 2048, 2047)[1] > 2 ** 30


def test_batches_have_image_bases_on_both_sides_of_4_gib():
    for name, (kinds, n, w, h, side) in lt.BATCHES.items():
        per = lt.tensor_bytes(kinds, w, h)[0 if side == "in" else 1]
        bases = [i * per for i in range(n)]
        assert per < lt.L and bases[-1] > lt.G4 > bases[1] and bases[-1] % lt.G4, (name, per)
        straddler = lt.G4 // per
        assert straddler * per <= lt.G4 < (straddler + 1) * per and straddler < n - 1, name     # the image that holds byte 2^32
    assert lt.tensor_bytes(("deconv",), 1024, 1020)[1] * 9 == 4812963840 > lt.G4 > lt.tensor_bytes(("deconv",), 1024, 1020)[1] * 8
    assert lt.tensor_bytes(("l0",), 4096, 2048)[1] * 16 == lt.G4                                 # 17 images: the last base is 2^32 itself


def test_nt_chains_write_exactly_the_bytes_that_select_nt_stores():
    for name, (kinds, n, w, h) in lt.NT_CHAINS.items():
        assert n * lt.tensor_bytes(kinds, w, h)[1] >= lt.NT_MIN_BYTES == 134217728, name
    kinds, n, w, h = lt.NT_CHAINS["conv"]
    assert n * lt.tensor_bytes(kinds, w, h)[1] == lt.NT_MIN_BYTES > (n - 1) * lt.tensor_bytes(kinds, w, h)[1]     # 2 x 64 MiB: the threshold itself


def test_gdn_lane_counts_have_a_second_and_a_third_chunk():
    assert lt.gdn_chunk(128) == 16777184 and lt.gdn_chunk(192) == 11184789
    for c in (128, 192):
        k = lt.gdn_chunk(c)
        assert k * c < lt.L <= (k + 22) * c + 4096
        assert (k + 300) * c > lt.L - 4096 and (2 * k + 1) * c > lt.G4 - 2 * 4096 - 2 * c


def test_rgb_batch_limit_is_87_images_of_4k():
    per = 3840 * 2160 * 3
    assert 87 * per == 2164838400 and 87 * per + 4 >= lt.L > 86 * per + 4
    assert 86 * 1920 * 1080 * 128 == 22826188800                    # the accepted side's output: left out, 22.8 GB


# ---- the ragged layout (host only) ----------------------------------------------------------------------------------------------------
def _layout(kind, sizes, layer, image):
    d = lt.desc(kind, 8, 8)
    cdescs = (CLayerDesc * 1)(d.to_c())
    n = len(sizes)
    ws = (ctypes.c_int32 * n)(*[w for w, _ in sizes])
    hs = (ctypes.c_int32 * n)(*[h for _, h in sizes])
    q = (ctypes.c_int64 * 8)()
    rc = _lib.lib().sicn_ragged_layout(cdescs, 1, ws, hs, n, layer, image, q)
    return rc, [int(v) for v in q]


def test_ragged_layout_gives_offsets_past_4_gib_as_they_are():
    sizes = lt.RAGGED_SIZES
    per = [w * h * 128 for w, h in sizes]
    want = [sum(per[:i]) for i in range(len(per))]
    assert want[2] == 4293918720 < lt.G4 < want[2] + per[2] and want[3] > lt.G4 and want[4] > want[3]
    for i, ((w, h), off) in enumerate(zip(sizes, want)):
        rc, q = _layout("conv", sizes, -1, i)
        assert rc == 0 and q[:5] == [w, h, 128, off, sum(per)], (i, q)
        rc, q = _layout("conv", sizes, 0, i)
        assert rc == 0 and q[:3] == [(w + 1) // 2, (h + 1) // 2, 128], (i, q)
    # the deconv's OUTPUT tensor past 2^32 the same way: inputs of half the size
    halves = lt.RAGGED_HALVES
    outs = [4 * w * h * 128 for w, h in halves]
    assert sum(outs[:2]) == 4292870144 < lt.G4 < sum(outs[:3])
    for i in range(len(halves)):
        rc, q = _layout("deconv", halves, 0, i)
        assert rc == 0 and q[:5] == [2 * halves[i][0], 2 * halves[i][1], 128, sum(outs[:i]), sum(outs)], (i, q)


@pytest.mark.parametrize("kind, w, h", [("conv", 4096, 4095), ("deconv", 2048, 2047), ("l0", 8192, 8190), ("rgb", 4096, 4095)])
def test_ragged_layout_refuses_an_image_of_exactly_l_bytes(kind, w, h):
    """one step under the limit is laid out; with one row more the image is exactly L bytes on one side of the layer: SICN_EINVAL,
    whichever image of the batch it is and whichever boundary is asked for"""
    assert max(lt.tensor_bytes((kind,), w, h)) < lt.L == max(lt.tensor_bytes((kind,), w, h + 1))
    for layer in (-1, 0):
        assert _layout(kind, [(6, 4), (w, h), (5, 3)], layer, 2)[0] == 0
        for sizes in ([(w, h + 1), (6, 4)], [(6, 4), (w, h + 1)]):
            assert _layout(kind, sizes, layer, 0)[0] == -22, (kind, sizes, layer)
