"""Inputs and a second statement of the formats for tests/test_codec_edges.py and tests/test_codec_edges_gpu.py (no tests here).

Three things:
  * container mode 4 restated in numpy from the comment block at the top of oracle/sicn_hyper_oracle.c (checkerboard sets, symbol
    order, class rule, stream geometry) and the normalisation rule (floor, bump to 1, largest first / lowest index on ties) —
    this part calls none of the oracle's functions;
  * the contents of the context-coder matrix (constant, uniform, checkerboard, one rare symbol, tied class maxima);
  * latents that drive chosen streams to the format's maximum rate of 12 bits per symbol (every hot symbol diluted to f = 1 by
    zeros elsewhere in the image) for mode 3 and mode 4, with the oracle's container cached per case.
"""
import functools

import numpy as np

from oracle import c_oracle

HEADER = 48
NCLS = 16
WSS = 16384                     # stream length of mode 4 (and the longest of mode 3)
CTX_TABLES = NCLS * 256         # bytes of the 16 class tables in a mode-4 container
CTX_LENS = HEADER + CTX_TABLES  # offset of the length table of a mode-4 container


# ---- mode 4 in numpy -------------------------------------------------------------------------------------------------------------
def ctx_masks(h, w):
    """(anchor mask, non-anchor mask) [h][w]: anchors are the pixels with (px + py) even."""
    py, px = np.mgrid[0:h, 0:w]
    anchor = (px + py) % 2 == 0
    return anchor, ~anchor


def ctx_geometry(h, w, c):
    """((anchor symbols, non-anchor symbols), (anchor streams, non-anchor streams)) of a [h][w][c] latent."""
    anchor, other = ctx_masks(h, w)
    nsym = (int(anchor.sum()) * c, int(other.sum()) * c)
    return nsym, tuple(-(-n // WSS) for n in nsym)


def ctx_classes(y, s):
    """Class of every element of y [h][w][c] given the scale map s: anchors s >> 3; non-anchors
    min(15, ((s >> 3) + (m >> 3) + 1) >> 1) with m the largest in-range 4-neighbour of y in the same channel."""
    h, w, _ = y.shape
    anchor, _ = ctx_masks(h, w)
    p = np.pad(y.astype(np.int64), ((1, 1), (1, 1), (0, 0)))        # symbols are >= 0: a zero border = "in-range neighbours only"
    m = np.maximum(np.maximum(p[:-2, 1:-1], p[2:, 1:-1]), np.maximum(p[1:-1, :-2], p[1:-1, 2:]))
    k0 = s.astype(np.int64) >> 3
    return np.where(anchor[:, :, None], np.minimum(k0, 15), np.minimum(15, (k0 + (m >> 3) + 1) >> 1))


def ctx_histograms(y, s):
    """[16][128] counts of (class, symbol) over the whole latent."""
    k = ctx_classes(y, s)
    return np.bincount((k * 128 + y.astype(np.int64)).reshape(-1), minlength=NCLS * 128).reshape(NCLS, 128).astype(np.uint32)


def ctx_set_order(y):
    """The symbols of y in coding order: anchors then non-anchors, pixels in raster order inside a set, channels fastest."""
    anchor, other = ctx_masks(*y.shape[:2])
    return np.concatenate([y[anchor].reshape(-1), y[other].reshape(-1)])


def floors(hist):
    """First step of the normalisation: floor(h * 4096 / n), a present symbol never below 1.  Returns (f, 4096 - sum f)."""
    hist = np.asarray(hist, np.int64)
    n = int(hist.sum())
    f = hist * 4096 // n
    f[(hist > 0) & (f == 0)] = 1
    return f, 4096 - int(f.sum())


def oracle_normalize(hist):
    hist = np.ascontiguousarray(hist, np.uint32)
    f = np.zeros(128, np.uint16)
    assert c_oracle.lib().sicl_or_normalize(c_oracle._ptr(hist), int(hist.sum()), c_oracle._ptr(f)) == 0
    return f


def ctx_container_fields(blob):
    """(header dwords [12], tables [16][128], stream lengths [n_streams]) of a mode-4 container."""
    head = np.frombuffer(blob[:HEADER], "<u4")
    ns = int(head[8])
    tables = np.frombuffer(blob[HEADER:CTX_LENS], "<u2").reshape(NCLS, 128)
    return head, tables, np.frombuffer(blob[CTX_LENS:CTX_LENS + 4 * ns], "<u4")


# ---- contents of the context-coder matrix ---------------------------------------------------------------------------------------
CTX_BIG = [(4, 64, 128), (1, 8193, 4), (37, 37, 192)]
CTX_SMALL = [(2, 2, 4), (3, 3, 4), (5, 1, 8), (1, 5, 8), (1, 1, 4)]
CTX_COUNTS = {(4, 64, 128): ((16384, 16384), (1, 1)), (1, 8193, 4): ((16388, 16384), (2, 1)),
              (37, 37, 192): ((131520, 131328), (9, 9)), (1, 1, 4): ((4, 0), (1, 0))}
TIE_A, TIE_B = 3, 5             # the tied symbols: below 8, so that no neighbour maximum leaves class 0


def tie_plan(shape, want_up):
    """Counts for the tie case on `shape`: symbols TIE_A and TIE_B `t` times each (the maxima of class 0) and `k` further symbols
    `r` times each, such that the floors miss 4096 from below (want_up: diff > 0) or from above (diff < 0) and the walk can settle
    it on one symbol.  The rare symbols go to non-anchor positions only, where they are nobody's context.  None if the shape has no
    such split (e.g. every count a multiple of n / 4096)."""
    h, w, c = shape
    n = h * w * c
    (na, nn), _ = ctx_geometry(h, w, c)
    rs = [1] + sorted({-(-int(fr * n) // 4096) for fr in (1.9, 2.9, 0.9)} - {0, 1})
    for r in rs:
        for k in range(0, 127):
            if k * r > nn or (n - k * r) % 2:
                continue
            t = (n - k * r) // 2
            if t <= r or 2 * t < na:
                continue
            hist = np.zeros(128, np.int64)
            hist[TIE_A] = hist[TIE_B] = t
            rare = [v for v in range(128) if v not in (TIE_A, TIE_B)][:k]
            hist[rare] = r
            f, diff = floors(hist)
            if (diff > 0 if want_up else diff < 0) and f[TIE_A] + diff > max(1, r * 4096 // n):
                return t, k, r, diff
    return None


def tie_latent(shape, want_up, rng):
    """(y, plan): the tie case, or the plain two-symbol split (plan None) where the shape admits no miss in that direction."""
    h, w, c = shape
    n = h * w * c
    plan = tie_plan(shape, want_up)
    t, k, r = plan[:3] if plan else (n // 2, 0, 0)
    anchor, other = ctx_masks(h, w)
    y = np.zeros(shape, np.uint8)
    na, nn = int(anchor.sum()) * c, int(other.sum()) * c
    rare = np.repeat(np.array([v for v in range(128) if v not in (TIE_A, TIE_B)][:k], np.uint8), r)
    pool = np.concatenate([np.full(t, TIE_A, np.uint8), np.full(n - t - rare.size, TIE_B, np.uint8)])
    rng.shuffle(pool)
    tail = np.concatenate([pool[na:], rare])                       # non-anchors: the rest of the pool and every rare symbol
    rng.shuffle(tail)
    y[anchor] = pool[:na].reshape(-1, c)
    if nn:
        y[other] = tail.reshape(-1, c)
    return y, plan


def _checkerboard(shape):
    anchor, _ = ctx_masks(*shape[:2])
    return np.where(anchor[:, :, None], 127, 0).astype(np.uint8) * np.ones(shape, np.uint8)


def _one_77(shape):
    y = np.zeros(shape, np.uint8)
    y.reshape(-1)[-1] = 77
    return y


CTX_CONTENTS = {                 # name -> (y, s) of one [h][w][c] image
    "zeros": lambda sh, rng: (np.zeros(sh, np.uint8), np.zeros(sh, np.uint8)),
    "y127-s127": lambda sh, rng: (np.full(sh, 127, np.uint8), np.full(sh, 127, np.uint8)),
    "y0-s127": lambda sh, rng: (np.zeros(sh, np.uint8), np.full(sh, 127, np.uint8)),
    "y127-s0": lambda sh, rng: (np.full(sh, 127, np.uint8), np.zeros(sh, np.uint8)),
    "uniform-s0": lambda sh, rng: (rng.integers(0, 128, sh, dtype=np.uint8), np.zeros(sh, np.uint8)),
    "uniform-uniform": lambda sh, rng: (rng.integers(0, 128, sh, dtype=np.uint8), rng.integers(0, 128, sh, dtype=np.uint8)),
    "checkerboard": lambda sh, rng: (_checkerboard(sh), np.zeros(sh, np.uint8)),
    "one-77": lambda sh, rng: (_one_77(sh), np.zeros(sh, np.uint8)),
    "tie-up": lambda sh, rng: (tie_latent(sh, True, rng)[0], np.zeros(sh, np.uint8)),
    "tie-down": lambda sh, rng: (tie_latent(sh, False, rng)[0], np.zeros(sh, np.uint8)),
}
# batches of three DIFFERENT contents (a wrong per-image stride shows); every content occurs at least once
CTX_BATCHES = [("zeros", "y127-s127", "y0-s127"), ("y127-s0", "uniform-s0", "uniform-uniform"),
               ("checkerboard", "one-77", "tie-up"), ("tie-down", "uniform-uniform", "y127-s0")]


@functools.lru_cache(maxsize=None)
def ctx_case(shape, batch):
    """(y [3][h][w][c], s [3][h][w][c], [oracle container] * 3) of one cell of the matrix; computed once, never modified."""
    rng = np.random.default_rng([sum(shape), batch])
    ys, ss = zip(*[CTX_CONTENTS[name](shape, rng) for name in CTX_BATCHES[batch]])
    y, s = np.stack(ys), np.stack(ss)
    y.setflags(write=False)
    s.setflags(write=False)
    wh = (shape[1] * 16, shape[0] * 16)
    return y, s, [c_oracle.ctx_encode(y[i], s[i], wh) for i in range(3)]


# ---- streams at the format's maximum rate -----------------------------------------------------------------------------------
RATE3 = {       # name -> (n symbols, stream length, hot streams); stream IRREGULAR is hot too, but with zeros mixed in
    "latency-form": (64 * 16384 + 1000, 16384, (0, 31, 64)),
    "two-table-form": (1300 * 8192 + 500, 8192, (0, 650, 1299, 1300)),
    "scan-form": (2049 * 8192 + 500, 8192, (0, 1024, 2048, 2049)),
}
IRREGULAR = 1
RING_WORDS = 4096               # csrc/k_codec_body.hpp: the LDS ring of a stream's 16-bit words
FLUSH_ABOVE = RING_WORDS - 4 * 64 - 128   # the encoders flush after a block of 4 steps that leaves more words than this pending


@functools.lru_cache(maxsize=None)
def rate3_case(name):
    """(latent [1][1][n], container of the oracle at the case's stream length, stream lengths).  Zeros but in the hot streams,
    which hold uniform 1..127: the image-wide table gives every hot symbol f = 1, i.e. 12 bits each.  All 64 lanes of such a stream
    renormalise in the same three steps of every four, so its pending words are always a multiple of 192: stream IRREGULAR holds
    uniform 0..127 instead — the zeros cost nothing and put the lanes out of step, so that flushed runs start and end off the multiples
    of 8 words and the pending words come closer to the ring's size."""
    n, ss, hot = RATE3[name]
    rng = np.random.default_rng(n)
    lat = np.zeros(n, np.uint8)
    for st in hot:
        a, b = st * ss, min(n, (st + 1) * ss)
        lat[a:b] = rng.integers(1, 128, b - a, dtype=np.uint8)
    lat[IRREGULAR * ss:(IRREGULAR + 1) * ss] = rng.integers(0, 128, ss, dtype=np.uint8)
    lat = lat.reshape(1, 1, n)
    lat.setflags(write=False)
    blob = c_oracle.codec_encode(lat, (0, 0), 3, stream_symbols=ss)
    ns = -(-n // ss)
    return lat, blob, np.frombuffer(blob[HEADER + 256:HEADER + 256 + 4 * ns], "<u4")


def assert_rate3_is_at_the_bound(name):
    """From the oracle's container alone: the hot symbols have f = 1, every full hot stream has exactly 1.5 ss + 256 bytes (three
    16-bit words per four symbols + the 64 final states — the format's maximum), every cold stream its 256 bytes of states."""
    n, ss, hot = RATE3[name]
    _, blob, lens = rate3_case(name)
    freq = np.frombuffer(blob[HEADER:HEADER + 256], "<u2")
    assert np.all(freq[1:] == 1) and freq[0] == 4096 - 127
    ns = -(-n // ss)
    assert lens.size == ns and ns - 1 in hot and IRREGULAR not in hot
    for st in range(ns):
        cnt = min(ss, n - st * ss)
        if st == IRREGULAR:
            # zeros are 1 symbol in 128 (mean ss / 128, standard deviation below sqrt(ss / 128) < 12: at most ss / 64 of them), every
            # other symbol costs 12 bits, less the up to 16 bits each of the 64 final states holds beyond its first 16
            assert 256 + 3 * (ss - ss // 64) // 2 - 128 <= lens[st] < 3 * ss // 2 + 256, (st, lens[st])
        elif st not in hot:
            assert lens[st] == 256, (st, lens[st])
        elif cnt == ss:
            assert lens[st] == 3 * ss // 2 + 256, (st, lens[st])
        else:       # the short tail: 12 bits per symbol, less the up to 16 bits each of the 64 final states holds beyond its first 16
            assert 256 + 3 * cnt // 2 - 128 <= lens[st] <= 256 + 3 * cnt // 2, (st, lens[st])
    return lens


def encoder_block_words(sym, freq):
    """The 16-bit words a rANS-W encoder emits in every block of 4 steps of one stream, in coding order (last block first): the
    container format's arithmetic (64 lanes, lane l codes symbols 256 q + 4 l + k in step 4 q + k, a lane emits a word when its
    state is >= f << 20), with nothing of the GPU's ring in it.  sum + 128 words are the stream."""
    freq = np.asarray(freq, np.uint64)
    cum = np.concatenate([[0], np.cumsum(freq)[:-1]]).astype(np.uint64)
    cnt = len(sym)
    blocks = -(-cnt // 256)
    pad = np.zeros(blocks * 256, np.int64)
    pad[:cnt] = sym
    pad = pad.reshape(blocks, 64, 4)
    act = (np.arange(blocks * 256) < cnt).reshape(blocks, 64, 4)
    x = np.full(64, 1 << 16, np.uint64)
    out = []
    for q in range(blocks - 1, -1, -1):
        w = 0
        for k in (3, 2, 1, 0):
            a, f, c = act[q, :, k], freq[pad[q, :, k]], cum[pad[q, :, k]]
            emit = a & (x >= (f << np.uint64(20)))
            w += int(emit.sum())
            x = np.where(emit, x >> np.uint64(16), x)
            fs = np.where(a, f, np.uint64(1))
            x = np.where(a, ((x // fs) << np.uint64(12)) + x % fs + c, x)
        out.append(w)
    return out


def ring_occupancy(words, flush_above):
    """The encoders' ring discipline on those counts: (most words ever pending, the 128 of the final states included; flushes before
    the final one; the word indices modulo 8 at which flushed runs begin or end)."""
    pending, most, flushes, pos, edges = 0, 0, 0, 0, set()
    for w in words:
        pending += w
        pos += w
        most = max(most, pending)
        if pending > flush_above:
            pending, flushes = 0, flushes + 1
            edges.add(-pos % 8)
    return max(most, pending + 128), flushes, edges | {-(pos + 128) % 8}


RATE4_VARIANTS = ("anchors", "non-anchors", "both")


@functools.lru_cache(maxsize=None)
def rate4_case(h):
    """Mode 4 on (h, 37, 192): (y [3], s [3], [oracle container] * 3).  s uniform; y zero but in the row bands [0, 6) and [h - 6, h),
    uniform 1..127 on (a) the anchors, (b) the non-anchors — the neighbour maxima stay 0 and the classes stay diluted — (c) both."""
    shape = (h, 37, 192)
    rng = np.random.default_rng(h)
    anchor, other = ctx_masks(h, 37)
    band = np.zeros((h, 37), bool)
    band[:6] = band[h - 6:] = True
    ys, ss = [], []
    for mask in (anchor, other, anchor | other):
        y = rng.integers(1, 128, shape, dtype=np.uint8)
        y[~(mask & band)] = 0
        ys.append(y)
        ss.append(rng.integers(0, 128, shape, dtype=np.uint8))
    y, s = np.stack(ys), np.stack(ss)
    y.setflags(write=False)
    s.setflags(write=False)
    return y, s, [c_oracle.ctx_encode(y[i], s[i], (37 * 16, h * 16)) for i in range(3)]


def assert_rate4_is_near_the_bound(h):
    """From the oracle's containers alone: the targeted streams come close to the 24832 bytes a stream can have."""
    _, _, blobs = rate4_case(h)
    (_, _), (na, nn) = ctx_geometry(h, 37, 192)
    lens = [ctx_container_fields(b)[2] for b in blobs]
    assert all(v.size == na + nn and int(v.max()) <= 3 * WSS // 2 + 256 for v in lens)
    a, b, c = lens
    if h == 200:
        assert a[0] >= 24000 and b[na] >= 24000, (a[0], b[na])
        assert min(c[0], c[na]) >= 20000 and min(c[na - 2], c[na + nn - 2]) >= 20000, (c[0], c[na], c[na - 2], c[na + nn - 2])
    else:
        assert a[na - 1] >= 14000 and b[na + nn - 1] >= 14000, (a[na - 2:na], b[-2:])   # the band split over the last two streams
    return lens
