"""The K map of layer 7's second weight image (csrc/k_rgb.hip: pack_l7_half, read by k_l7<1>), restated here next to pack_l7's.
Both images have the rows of the tap-product form (row = 4 (2 py + px) + r); they differ only in which channel a K byte stands for:
  pack_l7      [M tile 2][dx 3][half 2][row 16][64 B]: byte b = channel 64 (kg & 1) + 32 half + 16 (kg >> 1) + (b & 15), kg = b >> 4
  pack_l7_half [M tile 2][dx 3][row 16][64 B]:         byte b = channel b
No GPU and no library: the library's own packer is held to the oracle's bytes by tests/test_l7_live_half_gpu.py."""
import numpy as np


def _row_taps(tile, row):
    g, r = row >> 2, row & 3
    py, px = g >> 1, g & 1
    if r < 3:
        return (2 - py if tile == 0 else (3 if py else 0)), px, r
    return 4, px, ((2 if tile == 0 else -1) if py else tile)


def channel_full(half, b):
    kg = b >> 4
    return 64 * (kg & 1) + 32 * half + 16 * (kg >> 1) + (b & 15)


def channel_half(b):
    return b


def pack(w_okc, halves):
    """w_okc [3][5][5][128] -> the image of pack_l7 (halves = 2) or pack_l7_half (halves = 1)"""
    steps = 2 if halves == 2 else 1
    img = np.zeros((2, 3, steps, 16, 64), np.int8)
    for tile in range(2):
        for dx in range(3):
            for row in range(16):
                ky, px, c = _row_taps(tile, row)
                kx = 2 * dx - px
                if c < 0 or not 0 <= kx < 5:
                    continue
                for half in range(steps):
                    for b in range(64):
                        img[tile, dx, half, row, b] = w_okc[c, ky, kx, channel_full(half, b) if halves == 2 else channel_half(b)]
    return img


def test_every_channel_of_the_first_half_once_per_column_shift():
    assert sorted(channel_half(b) for b in range(64)) == list(range(64))
    # lane group kg = b >> 4 reads chunk kg of region 0: 16 bytes (kg & 1) of the 32-channel group kg >> 1
    assert all(channel_half(b) == 32 * ((b >> 4) >> 1) + 16 * ((b >> 4) & 1) + (b & 15) for b in range(64))
    # the full image covers all 128 channels once per column shift, over its two K steps
    assert sorted(channel_full(h, b) for h in range(2) for b in range(64)) == list(range(128))


def test_half_image_is_the_full_images_first_half():
    rng = np.random.default_rng(7)
    w = rng.integers(-8, 8, (3, 5, 5, 128)).astype(np.int8)
    full, half = pack(w, 2), pack(w, 1)
    assert half.nbytes == 6144 and full.nbytes == 12288
    where = {channel_full(h, b): (h, b) for h in range(2) for b in range(64)}
    for ch in range(64):
        h, b = where[ch]
        assert np.array_equal(half[:, :, 0, :, ch], full[:, :, h, :, b]), ch
    # with the channels 64 .. 127 dead (what the live-channel plan guarantees) the two images hold the same products
    w[..., 64:] = 0
    x = rng.integers(0, 128, 128).astype(np.int64)
    x_dead = x.copy()
    x_dead[64:] = rng.integers(0, 256, 64)          # whatever the planes nobody wrote hold
    full = pack(w, 2).astype(np.int64)
    bx = np.array([[x_dead[channel_full(h, b)] for b in range(64)] for h in range(2)])
    t_full = np.einsum("tdhrb,hb->tdr", full, bx)
    t_half = np.einsum("tdrb,b->tdr", pack(w, 1)[:, :, 0].astype(np.int64), x[:64])
    assert np.array_equal(t_full, t_half)
