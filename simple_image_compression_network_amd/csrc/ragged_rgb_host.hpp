// The packed-K form of a ragged net's RGB ends (include/sicn_ragged_rgb.h, k_ragged_rgb.hip): which weight sits at which byte of
// which K step, and the two weight images.  Plain C++: the library and tests/cpp/ragged_rgb_pack_check.cpp both include this file.
//
// Conv 3 -> N.  The patch is RGBX dwords, so the five taps of kernel row ky at output column x are the 20 bytes from pixel 2x on.
// K is one 32-byte group per kernel row — 5 pixels x RGBX, then three pixel slots — and two kernel rows make one 64-byte K step:
//   byte b of K step s  <->  ky = 2 s + (b >> 5), kx = (b & 31) >> 2, c = b & 3
// real where ky < 5, kx < 5 and c < 3.  The X byte, the slots 5 .. 7 and the second half of step 2 carry ZERO WEIGHTS: whatever
// data the patch holds there is multiplied by 0.  3 K steps where the zero-padded form walks 25.
// Image: [block of 64 channels][K step 3][tile 4][row 16][64 B]; row rho of tile j of block J is channel
// 64 J + 16 (rho >> 2) + 4 j + (rho & 3), as pack_any has it, so that C/D row 4 g + r of tile j is channel 64 J + 16 g + 4 j + r.
//
// Deconv N -> 3.  One A tile carries all four phases: row 4 phase + c (phase = 2 qy + qx, c < 3) of tap offset (dy, dx) in
// {0, 1, 2}^2 holds W[c][ky = 2 (dy - qy) + qy][kx = 2 (dx - qx) + qx][.] where dy >= qy and dx >= qx, and zeros elsewhere; rows
// 4 phase + 3 are zero.  Offset (dy, dx) is patch pixel (ly + dy, lx + dx) of position (ly, lx): any_tile's (ly + qy + iy,
// lx + qx + ix) with ky = 2 iy + qy.  9 offsets where the four phases walk 9 + 6 + 6 + 4 taps, each over its own patch.
// Image: [offset dy * 3 + dx][64-channel chunk][row 16][64 B], zero for channels >= N.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sicn {

constexpr int RGB_CONV_KSTEPS = 3;
constexpr int RGB_DECONV_OFFSETS = 9;

struct RgbConvSlot {
    int ky, kx, c;
    bool real;
};
inline RgbConvSlot rgb_conv_slot(int step, int byte)
{
    const int ky = 2 * step + (byte >> 5), kx = (byte & 31) >> 2, c = byte & 3;
    return RgbConvSlot{ky, kx, c, ky < 5 && kx < 5 && c < 3};
}
inline int rgb_conv_channel(int J, int j, int rho) { return 64 * J + 16 * (rho >> 2) + 4 * j + (rho & 3); }
inline size_t rgb_conv_bytes(int cout) { return (size_t)((cout + 63) / 64) * RGB_CONV_KSTEPS * 4 * 1024; }

// w_okc: [cout][75], k = (ky * 5 + kx) * 3 + c
inline void pack_rgb_conv(const int8_t *w_okc, int cout, int8_t *dst)
{
    const int nblk = (cout + 63) / 64;
    for (int J = 0; J < nblk; J++)
        for (int s = 0; s < RGB_CONV_KSTEPS; s++)
            for (int j = 0; j < 4; j++)
                for (int rho = 0; rho < 16; rho++) {
                    const int o = rgb_conv_channel(J, j, rho);
                    int8_t *row = dst + ((((size_t)J * RGB_CONV_KSTEPS + s) * 4 + j) * 16 + rho) * 64;
                    for (int b = 0; b < 64; b++) {
                        const RgbConvSlot k = rgb_conv_slot(s, b);
                        row[b] = (k.real && o < cout) ? w_okc[(size_t)o * 75 + (k.ky * 5 + k.kx) * 3 + k.c] : 0;
                    }
                }
}

struct RgbDeconvRow {
    int phase, c, ky, kx;
    bool real;
};
inline RgbDeconvRow rgb_deconv_row(int offset, int row)
{
    const int dy = offset / 3, dx = offset - 3 * dy;
    const int phase = row >> 2, c = row & 3, qy = phase >> 1, qx = phase & 1;
    const int ky = 2 * (dy - qy) + qy, kx = 2 * (dx - qx) + qx;
    return RgbDeconvRow{phase, c, ky, kx, c < 3 && dy >= qy && dx >= qx};
}
inline size_t rgb_deconv_bytes(int cin) { return (size_t)RGB_DECONV_OFFSETS * ((cin + 63) / 64) * 1024; }

// w_okc: [3][25 * cin], k = (ky * 5 + kx) * cin + channel
inline void pack_rgb_deconv(const int8_t *w_okc, int cin, int8_t *dst)
{
    const int nchunk = (cin + 63) / 64;
    for (int t = 0; t < RGB_DECONV_OFFSETS; t++)
        for (int n = 0; n < nchunk; n++)
            for (int rho = 0; rho < 16; rho++) {
                const RgbDeconvRow r = rgb_deconv_row(t, rho);
                int8_t *row = dst + (((size_t)t * nchunk + n) * 16 + rho) * 64;
                for (int b = 0; b < 64; b++) {
                    const int ch = n * 64 + b;
                    row[b] = (r.real && ch < cin) ? w_okc[(size_t)r.c * 25 * cin + (size_t)(r.ky * 5 + r.kx) * cin + ch] : 0;
                }
            }
}

}  // namespace sicn
