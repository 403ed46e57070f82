"""CPU side of the coder edge tests (no GPU needed): container mode 4 stated a second time, in numpy, from the comment block at the top
of oracle/sicn_hyper_oracle.c (tests/codec_edge_cases.py), against the C oracle's containers for the shapes and contents of the GPU
matrix in tests/test_codec_edges_gpu.py; and the oracle-only facts the GPU tests of the maximum-rate streams rest on."""
import numpy as np
import pytest

import codec_edge_cases as ce
from oracle import c_oracle


@pytest.mark.parametrize("shape", list(ce.CTX_COUNTS))
def test_ctx_geometry_counts(shape):
    nsym, nst = ce.ctx_geometry(*shape)
    assert (nsym, nst) == ce.CTX_COUNTS[shape]
    if shape == (1, 1, 4):
        assert nst == (1, 0)                                        # no non-anchors: the second decode launch is skipped


def test_ctx_set_order_is_the_header_comments_formula():
    """Raster order inside a set, as boolean-mask indexing gives it, is the closed form of the comment: pixel j of a set lies in row
    pair r = j / W at t = j % W, the even row first."""
    for h, w in ((1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (4, 7), (7, 4), (37, 37)):
        a, b = (w + 1) // 2, w // 2
        anchor, other = ce.ctx_masks(h, w)
        for mask, first, second in ((anchor, lambda t: 2 * t, lambda t: 2 * (t - a) + 1), (other, lambda t: 2 * t + 1, lambda t: 2 * (t - b))):
            split = a if mask is anchor else b
            pix = []
            for j in range(int(mask.sum())):
                r, t = divmod(j, w)
                pix.append((2 * r, first(t)) if t < split else (2 * r + 1, second(t)))
            assert pix == [tuple(p) for p in np.argwhere(mask)]
        assert int(anchor.sum()) == (h // 2) * w + (a if h % 2 else 0) and int(other.sum()) == (h // 2) * w + (b if h % 2 else 0)


@pytest.mark.parametrize("batch", range(len(ce.CTX_BATCHES)))
@pytest.mark.parametrize("shape", ce.CTX_BIG + ce.CTX_SMALL)
def test_ctx_oracle_tables_and_streams_equal_the_numpy_statement(shape, batch):
    y, s, blobs = ce.ctx_case(shape, batch)
    nsym, nst = ce.ctx_geometry(*shape)
    for i, blob in enumerate(blobs):
        head, tables, lens = ce.ctx_container_fields(blob)
        assert head[:2].tolist() == [0x4C434953, 1 | (4 << 16)] and head[4:8].tolist() == [shape[1], shape[0], shape[2], y[i].size]
        assert int(head[8]) == sum(nst) == lens.size and int(head[9]) == ce.WSS
        assert int(head[10]) == int(lens.sum()) == len(blob) - ce.CTX_LENS - 4 * lens.size
        hist = ce.ctx_histograms(y[i], s[i])
        assert int(hist.sum()) == sum(nsym)
        for k in range(ce.NCLS):
            want = ce.oracle_normalize(hist[k]) if hist[k].any() else np.zeros(128, np.uint16)
            assert np.array_equal(tables[k], want), (ce.CTX_BATCHES[batch][i], k)
        # the streams of a set cover its symbols: a stream of cnt symbols has its 64 states and at most one word per symbol
        order = ce.ctx_set_order(y[i])
        assert order.size == sum(nsym) and np.array_equal(np.sort(order), np.sort(y[i].reshape(-1)))
        cnts = [min(ce.WSS, n - q * ce.WSS) for n, k in zip(nsym, nst) for q in range(k)]
        assert all(256 <= int(v) <= 256 + 2 * c and v % 2 == 0 for v, c in zip(lens, cnts))
        back, _ = c_oracle.ctx_decode(blob, s[i])
        assert np.array_equal(back, y[i])


@pytest.mark.parametrize("shape", ce.CTX_BIG)
def test_tie_case_walks_in_both_directions_and_takes_the_lowest_index(shape):
    """Two symbols with equal counts, both the class maximum, and a floor sum that misses 4096: the correction goes to the LOWER of
    the two, when the sum is short (diff > 0) and when it is long (diff < 0).  A long sum needs single-count symbols (each bumped from
    0 to 1); on a latent of more than 4096 symbols these can only make it long, so the short sum comes from one symbol with a few
    occurrences whose floor loses a fraction, like those of the tied pair."""
    rng = np.random.default_rng(5)
    for want_up in (True, False):
        y, plan = ce.tie_latent(shape, want_up, rng)
        assert plan is not None
        t, k, r, diff = plan
        hist = ce.ctx_histograms(y, np.zeros_like(y))
        assert not hist[1:].any()                                   # everything in class 0
        assert hist[0, ce.TIE_A] == hist[0, ce.TIE_B] == t == hist[0].max() and int((hist[0] == r).sum()) == k
        f, d = ce.floors(hist[0])
        assert d == diff and (d > 0) == want_up and d != 0 and f[ce.TIE_A] == f[ce.TIE_B]
        got = ce.oracle_normalize(hist[0])
        want = f.copy()
        want[ce.TIE_A] += d
        assert np.array_equal(got, want) and got[ce.TIE_B] == f[ce.TIE_B]


def test_one_rare_symbol_gets_frequency_one_beside_4095():
    y, s = ce.CTX_CONTENTS["one-77"]((37, 37, 192), None)
    _, tables, _ = ce.ctx_container_fields(c_oracle.ctx_encode(y, s))
    # the last pixel (36, 36) is an anchor: its two neighbours' zeros are coded in class ((77 >> 3) + 1) >> 1 = 5, a table with f = 4096
    assert tables[0, 0] == 4095 and tables[0, 77] == 1 and tables[5, 0] == 4096 and int(tables.sum()) == 2 * 4096


def test_checkerboard_puts_every_non_anchor_in_class_eight():
    y, s = ce.CTX_CONTENTS["checkerboard"]((3, 3, 4), None)
    k = ce.ctx_classes(y, s)
    anchor, other = ce.ctx_masks(3, 3)
    assert np.all(k[anchor] == 0) and np.all(k[other] == (127 // 8 + 1) // 2)
    _, tables, _ = ce.ctx_container_fields(c_oracle.ctx_encode(y, s))
    assert tables[0, 127] == 4096 and tables[8, 0] == 4096 and int(tables.sum()) == 2 * 4096   # two tables with f = 4096


@pytest.mark.parametrize("name", list(ce.RATE3))
def test_max_rate_mode3_streams_are_at_the_bound_and_round_trip(name):
    """What the GPU tests of the same name rely on, from the oracle alone: the hot streams have exactly 1.5 ss + 256 bytes.  In words:
    12288 + 128 at ss = 16384 — the encoder's ring of 4096 words is flushed whenever more than 3712 are pending, so such a stream
    crosses the threshold at least three times, a 7-bit stream once."""
    n, ss, hot = ce.RATE3[name]
    lens = ce.assert_rate3_is_at_the_bound(name)
    assert int(lens.max()) // 2 == 3 * ss // 4 + 128
    lat, blob, _ = ce.rate3_case(name)
    back, _ = c_oracle.codec_decode(blob)
    assert np.array_equal(back, lat)


@pytest.mark.parametrize("h", [200, 201])
def test_max_rate_mode4_streams_are_near_the_bound_and_round_trip(h):
    ce.assert_rate4_is_near_the_bound(h)
    y, s, blobs = ce.rate4_case(h)
    for i in range(3):
        back, _ = c_oracle.ctx_decode(blobs[i], s[i])
        assert np.array_equal(back, y[i])


@pytest.mark.parametrize("name", list(ce.RATE3))
def test_max_rate_streams_press_on_the_ring_margin(name):
    """The encoders' ring discipline (csrc/k_codec_body.hpp: flush after a block that leaves more than RING_WORDS - 4 * 64 - 128 words
    pending, then the 128 words of the final states) replayed on the CPU over the word counts of the format's own arithmetic, which
    reproduce the oracle's stream lengths.  What the GPU tests on these streams can and cannot see:
      * the hot streams wrap the 4096-word ring three times, a stream at 7 bits per symbol — the densest an older GPU test codes — once;
      * the regular hot streams always flush runs that begin and end at multiples of 8 words (64 lanes in step: 192 words a block);
        the irregular one begins and ends runs off those multiples, the ragged heads and tails of ring_flush;
      * a threshold of RING_WORDS - 64 would overwrite pending words of these streams;
      * a block of 4 steps never emits more than 192 words (a lane gains at most 12 bits a symbol and sheds 16 a word: three words in
        four steps), so every threshold up to RING_WORDS - 192 is a working one, RING_WORDS - 4 * 64 included: the margin in the
        code is safe by 192 words, and no valid input can tell such thresholds apart."""
    n, ss, hot = ce.RATE3[name]
    lat, blob, lens = ce.rate3_case(name)
    freq = np.frombuffer(blob[ce.HEADER:ce.HEADER + 256], "<u2")
    flat = lat.reshape(-1)
    caught = False
    for st in sorted(set(hot) | {ce.IRREGULAR}):
        words = ce.encoder_block_words(flat[st * ss:(st + 1) * ss], freq)
        assert 2 * (sum(words) + 128) == lens[st] and max(words) <= 192
        most, flushes, edges = ce.ring_occupancy(words, ce.FLUSH_ABOVE)
        assert most <= ce.FLUSH_ABOVE + 192 <= ce.RING_WORDS
        if len(words) == ss // 256:                                 # a full stream
            assert flushes == (3 if ss == 16384 else 1)
            assert (edges == {0}) if st in hot else (edges - {0}), (st, edges)
            assert ce.ring_occupancy(words, ce.RING_WORDS - 4 * 64)[0] <= ce.RING_WORDS
            caught |= ce.ring_occupancy(words, ce.RING_WORDS - 64)[0] > ce.RING_WORDS
    assert caught
    rng = np.random.default_rng(0)
    seven = rng.integers(1, 128, 16384)                              # uniform over 1..127: 7 bits per symbol
    f7 = ce.oracle_normalize(np.bincount(seven, minlength=128))
    w7 = ce.encoder_block_words(seven, f7)
    assert ce.ring_occupancy(w7, ce.FLUSH_ABOVE)[1] == 1
