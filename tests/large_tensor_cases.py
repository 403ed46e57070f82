"""Shapes, weights, band arithmetic and byte arithmetic shared by tests/test_large_tensors.py (no GPU) and
tests/test_large_tensors_gpu.py (no tests here).

The limits of include/sicn.h: one image's input and output stay below L = 2^31 bytes per layer; a batch or a ragged tensor as a whole
may pass 2^32.  The C oracle cannot run an image of 2 GiB, so a result of that size is held to two other things:
  windows  a crop of at most 40 x 24 input pixels goes through the oracle's direct form, layer by layer, and is compared where the
           receptive field of an output lies inside the crop or at a true edge of the image (`window`, `window_positions`);
  bands    the input is cut into horizontal bands, each one runs through the same layers as a small image of its own, and the rows of
           the big result whose receptive field through the whole chain lies inside the band, or at a true edge, must be the band's
           rows, byte for byte (`band_plan`).  The bands of a plan overlap by the chain's margin, so every output row is compared.
Both rest on one function, `valid`: rows [a, b) of an image of H rows, run alone, give which rows of the chain's output exactly.  It is
one-dimensional and serves columns as well as rows.  A conv 5/2/2 reads input rows 2o - 2 .. 2o + 2 for its output row o, so an output
row next to a cut is wrong (1 row); a deconv 5/2/2 adds input row i into output rows 2i - 2 .. 2i + 2, so the output row below a cut
and the two above one are wrong; behind another layer the wrong rows of its input count as cut off.  A band begins at a multiple of 2^(number of convs),
so that its rows keep their parity through the chain.  tests/test_large_tensors.py holds `valid` and `band_plan` to the oracle."""
import functools

import numpy as np

import live_geometry_cases as lg
from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import LayerDesc

L = 1 << 31                                 # the first image size in bytes that a specialised kernel refuses (csrc/k_common.hpp OOB)
G4 = 1 << 32
NT_MIN_BYTES = 128 << 20                    # csrc/k_common.hpp nt_store_wanted: a launch that writes this much stores non-temporal
GUARD = 4096                                # known bytes in front of and behind every output

# kind: (cin, cout, SIMD, PE, transposed); the four kinds of live_geometry_cases.KINDS keep their names, weights and words
KINDS = {k: (128,) + v for k, v in lg.KINDS.items()}
KINDS.update({"l0": (3, 128, 3, 8, 0), "deconv192": (192, 128, 12, 16, 1), "conv64": (64, 64, 8, 16, 0), "conv16": (128, 16, 8, 16, 0)})


def desc(kind, w, h):
    cin, cout, simd, pe, tr = KINDS[kind]
    return LayerDesc.make(cin, cout, simd, pe, w, h, tr)


def chain_descs(kinds, w, h):
    """descriptors of `kinds` one behind the other, the first one on a w x h input"""
    if all(k in lg.KINDS for k in kinds):
        return lg.chain_descs(kinds, w, h)
    out = []
    for k in kinds:
        out.append(desc(k, w, h))
        w, h = out[-1].OFM_ROW, out[-1].OFM_COL
    return out


@functools.lru_cache(maxsize=None)
def weights(kind, seed, n_dead=0):
    """(W[o][ky][kx][c] int8 in -8 .. 7, bias int8 per channel), as live_geometry_cases.weights, which serves its own kinds"""
    if kind in lg.KINDS:
        return lg.weights(kind, seed, n_dead)
    assert n_dead == 0
    cin, cout = KINDS[kind][:2]
    rng = np.random.default_rng([seed, 50 + sorted(KINDS).index(kind)])
    w = rng.integers(-8, 8, (cout, 5, 5, cin)).astype(np.int8)
    b = rng.integers(-128, 128, cout).astype(np.int8)
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


def words(kind, w):
    if kind in lg.KINDS:
        return lg.words(kind, w)
    return sicn_ref.pack_finn_tiles(w, KINDS[kind][2], KINDS[kind][3])


def chain_weights(kinds, seed, n_dead=0):
    """layer 0 dense; layer l > 0 with n_dead dead input channels (live_geometry_cases.chain_weights)"""
    return [weights(k, seed + l, n_dead if l else 0) for l, k in enumerate(kinds)]


def transposed(kinds):
    return [KINDS[k][4] for k in kinds]


# ---- rows (or columns) through a chain ------------------------------------------------------------------------------------------------
def out_size(kinds, n):
    for tr in transposed(kinds):
        n = 2 * n if tr else (n + 1) // 2
    return n


def alignment(kinds):
    """a band or a window begins at a multiple of this"""
    return max(2, 1 << sum(1 for tr in transposed(kinds) if not tr))


def valid(kinds, a, b, n):
    """rows [a, b) of n, run through the chain as an image of b - a rows: (lo, hi, off) — rows [lo, hi) of that run's last output
    are rows [off + lo, off + hi) of the whole image's last output.  a is a multiple of alignment(kinds)."""
    assert 0 <= a < b <= n and a % alignment(kinds) == 0, (a, b, n)
    top, bottom = a == 0, b == n                       # a true edge: the band's zero padding is the layer's own
    lo, hi, off, size = 0, b - a, a, b - a
    for tr in transposed(kinds):
        if tr:
            # output y sums inputs (y - 2) / 2 .. (y + 2) / 2: all of them in [lo, hi)
            lo, hi, off, size = (0 if top else 2 * lo + 1), (2 * size if bottom else 2 * hi - 2), 2 * off, 2 * size
        else:
            assert off % 2 == 0
            size = (size + 1) // 2
            # output o reads 2o - 2 .. 2o + 2: all of them in [lo, hi)
            lo, hi, off = (0 if top else (lo + 3) // 2), (size if bottom else (hi - 3) // 2 + 1), off // 2
        hi = max(hi, lo)
    return lo, hi, off


def band_plan(kinds, n, n_bands):
    """[(a, b, p, q, r)]: input rows [a, b) run alone; rows [p, q) of the big output are rows [r, r + q - p) of that run's output.
    The [p, q) are n_bands (or fewer, for a small n) ranges that tile the output."""
    al, total = alignment(kinds), out_size(kinds, n)
    cuts = sorted({total * k // n_bands for k in range(n_bands + 1)})
    plan = []
    for p, q in zip(cuts, cuts[1:]):
        a, b = p, q                                    # back through the chain, then widened until `valid` covers [p, q)
        for tr in reversed(transposed(kinds)):
            a, b = (a // 2 - 1, (b + 1) // 2 + 1) if tr else (2 * a - 2, 2 * b + 1)
        a, b = max(a, 0) // al * al, max(min(b, n), 1)
        while True:
            lo, hi, off = valid(kinds, a, b, n)
            if off + lo <= p and off + hi >= q:
                break
            assert (off + lo > p and a > 0) or (off + hi < q and b < n), (kinds, n, p, q, a, b)
            if off + lo > p:
                a -= al
            if off + hi < q:
                b += 1
        plan.append((a, b, p, q, p - off))
    return plan


def window(kinds, size, at, extent):
    """the input range [a, b) of at most `extent` whose run holds output index `at` of an axis of `size` inputs in its valid part:
    (a, b, lo, hi, off) as `valid` gives them"""
    al, total = alignment(kinds), out_size(kinds, size)
    assert 0 <= at < total
    c = at
    for tr in reversed(transposed(kinds)):
        c = c // 2 if tr else 2 * c
    extent = min(extent, size)
    a = min(max(c - extent // 2, 0) // al * al, (size - extent + al - 1) // al * al)
    b = min(a + extent, size)
    lo, hi, off = valid(kinds, a, b, size)
    assert off + lo <= at < off + hi, (kinds, size, at, a, b, lo, hi, off)
    return a, b, lo, hi, off


WINDOW_W, WINDOW_H = 40, 24


def window_positions(kinds, w, h, seed, last_rows=False, n_random=6):
    """output positions (oy, ox) that a case's windows hold: the four corners (the last one holds the tensor's last byte), the NHWC
    byte offsets 2^28, 2^29 and 2^30 where the output has them, a window at the last rows away from the corners (behind a GROUP or
    PHASE intermediate the halo rows above IH alias the next plane), and seeded random ones"""
    ow, oh = out_size(kinds, w), out_size(kinds, h)
    c = KINDS[kinds[-1]][1]
    at = [(0, 0), (0, ow - 1), (oh - 1, 0), (oh - 1, ow - 1)]
    for e in (28, 29, 30):
        if (1 << e) < oh * ow * c:
            at.append(((1 << e) // (ow * c), (1 << e) % (ow * c) // c))
    if last_rows:
        at.append((oh - 1, ow // 2))
    rng = np.random.default_rng([seed, w, h])
    at += [(int(rng.integers(0, oh)), int(rng.integers(0, ow))) for _ in range(n_random)]
    return at


def oracle_chain(kinds, wb, x, gdn=None):
    """one image x [h][w][c] through the oracle's direct form, layer by layer; gdn: per layer None or (beta, gamma, inverse, shift),
    the activation in place of that layer's ReLU"""
    for l, (k, d, (w, b)) in enumerate(zip(kinds, chain_descs(kinds, x.shape[1], x.shape[0]), wb)):
        if gdn is not None and gdn[l] is not None:
            x = c_oracle.gdn(c_oracle.run_layer_preact(d, words(k, w), b, x, threads=16), *gdn[l])
        else:
            x = c_oracle.run_layer(d, words(k, w), b, x, form="direct", threads=16)
    return x


def stitched(kinds, n_bands, run, x):
    """the chain's output put together from the bands of band_plan, each run alone by `run`"""
    out = None
    for a, b, p, q, r in band_plan(kinds, x.shape[0], n_bands):
        y = run(np.ascontiguousarray(x[a:b]))
        if out is None:
            out = np.zeros((out_size(kinds, x.shape[0]),) + y.shape[1:], np.uint8)
        out[p:q] = y[r:r + q - p]
    return out


def first_difference(got, want):
    """None, or (row, x, channel) of the first differing byte of two [rows][w][c] arrays (numpy or torch)"""
    if hasattr(got, "cpu"):
        import torch
        if torch.equal(got, want):
            return None
        rows = torch.nonzero((got != want).flatten(1).any(1))
        y = int(rows[0])
        got, want, base = got[y:y + 1].cpu().numpy(), want[y:y + 1].cpu().numpy(), y
    else:
        if np.array_equal(got, want):
            return None
        base = 0
    y, x, c = (int(v) for v in np.argwhere(got != want)[0])
    return base + y, x, c


def check_bands(kinds, in_rows, n_bands, big_out, run_band, what):
    """every row of big_out [OH][OW][C] (numpy or torch) against run_band(a, b), the chain's output for input rows [a, b) run alone"""
    seen = 0
    for a, b, p, q, r in band_plan(kinds, in_rows, n_bands):
        y = run_band(a, b)
        bad = first_difference(big_out[p:q], y[r:r + q - p])
        if bad is not None:
            raise AssertionError(f"{what}: output rows {p} .. {q - 1} are not those of input rows {a} .. {b - 1} run alone; first at "
                                 f"(row {p + bad[0]}, x {bad[1]}, channel {bad[2]}): got {int(big_out[p + bad[0], bad[1], bad[2]])} "
                                 f"want {int(y[r + bad[0], bad[1], bad[2]])}")
        assert p == seen, (p, seen)
        seen = q
    assert seen == big_out.shape[0], (seen, big_out.shape)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
# A. one image just under the limit.  name: (kinds, W, H of the input, options, plan kind, plan family, the side that meets the
# limit, its bytes below L).  Plan kind and family are sicn_debug_plan's out[2] and out[3] (include/sicn.h).
SINGLE = {
    "conv-wide": (("conv",), 4096, 4095, {}, 1, 2, "in", 524288),
    "deconv-wide": (("deconv",), 2048, 2047, {}, 2, 2, "out", 1048576),
    "l0": (("l0",), 8192, 8190, {}, 3, 0, "out", 524288),
    "l7": (("rgb",), 4096, 4095, {}, 4, 0, "in", 524288),
    "conv192-pipelined": (("conv192",), 4096, 4095, {}, 1, 1, "in", 524288),
    "deconv192-pipelined": (("deconv192",), 2048, 2047, {}, 2, 1, "out", 1048576),
    "conv64-any": (("conv64",), 8192, 4095, {}, 5, 0, "in", 524288),
    "conv16-generic": (("conv16",), 4096, 4095, {"force_generic": 1}, 0, 0, "in", 524288),
}
# two chains with the internal layouts at the limit: (kinds, W, H, dead channels of the consumer, IGDN on the first layer)
CHAINS = {
    "l0-conv": (("l0", "conv"), 8192, 8190, 0, False),
    "deconv-l7": (("deconv", "rgb"), 2048, 2047, 0, False),
    "deconv-l7-half": (("deconv", "rgb"), 2048, 2047, 80, False),
}
# C. image bases on both sides of 2^32: (kinds, images, W, H, the tensor whose bases pass 2^32).  One image more than the 9 and 17 that
# first pass 2^32 with these sizes: of 9 x 534 773 760 bytes the last BASE is 4 278 190 080, still below 2^32, and of 17 x 2^28 the only
# base that is not below 2^32 is 2^32 itself; with 10 and 18 the last image begins beyond 2^32, at no multiple of it, and the one
# before it holds byte 2^32 inside or begins on it.
BATCHES = {
    "conv-wide": (("conv",), 10, 2048, 2040, "in"),
    "deconv-wide": (("deconv",), 10, 1024, 1020, "out"),
    "l0": (("l0",), 18, 4096, 2048, "out"),
    "l7": (("rgb",), 18, 2048, 1024, "in"),
}
# F. NT stores at the smallest size that selects them: (kinds, images, W, H)
NT_CHAINS = {"conv": (("conv", "conv"), 2, 2048, 1024), "deconv": (("deconv", "rgb"), 2, 512, 512)}
# D. ragged: the images of the 128-channel tensor that passes 2^32, (W, H) at that tensor
RAGGED_SIZES = [(4096, 4095), (4096, 4095), (256, 64), (70, 38), (5, 3)]
# the deconv's inputs, for an output that passes 2^32 the same way: (4096, 4094) twice, then 256 x 66 from 4 292 870 144 on (256 x 64
# would end on 2^32 itself)
RAGGED_HALVES = [(2048, 2047), (2048, 2047), (128, 33), (35, 19), (3, 2)]


def tensor_bytes(kinds, w, h):
    """(input bytes, output bytes of every layer) of one image"""
    ds = chain_descs(kinds, w, h)
    return [int(np.prod(ds[0].in_shape, dtype=np.int64))] + [int(np.prod(d.out_shape, dtype=np.int64)) for d in ds]


def gdn_chunk(c):
    """positions per launch of sicn_gdn_apply (csrc/sicn_abi.hip gdn_apply_lanes)"""
    return (L - 4096) // c


def gdn_params(c, seed):
    rng = np.random.default_rng([seed, c])
    beta = rng.integers(1, 65536, c).astype(np.uint32)
    gamma = rng.integers(0, 128, (c, c)).astype(np.uint8)
    gamma[rng.random((c, c)) < 0.5] = 0
    return beta, gamma
