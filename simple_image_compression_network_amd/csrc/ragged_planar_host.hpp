// The planar RGB boundaries of a ragged net (include/sicn_ragged_planar.h): where the bytes of a [3][h][w] image lie, how the conv
// 3 -> N loader reads a quad of them and how the deconv N -> 3 epilogue places a pixel.  Everything here is SICN_HD
// (k_ragged_common.hpp): the planar kernels of k_ragged_rgb.hip evaluate it on the device and tests/cpp/ragged_planar_check.cpp replays
// it on the host over byte arrays of exactly the permitted size.
//
// The loader.  A quad is 4 pixels of one patch row: one 4-byte window from each of the three planes, plane c at
// im + c h w + iy w + ix.  h w is arbitrary, so the three windows have three byte phases.  A window at phase sh lies in the aligned
// dwords a0 (always) and a0 + 4 (where sh != 0); a dword is LOADED ONLY WHERE IT OVERLAPS THE TENSOR [lo, hi) — with a 4-byte
// aligned tensor nothing before its first byte and nothing beyond its size rounded up to a multiple of 4 is touched — and reads as
// zero elsewhere.  alignbyte brings the window to one dword per plane (R0 R1 R2 R3 / G.. / B..), two byte permutes interleave R
// with G and four more add B and the zero X byte: the four RGBX dwords rgb_conv_tile's K layout reads.  Columns outside the image
// are zeroed afterwards, so whatever the window met there — the neighbouring row, plane or image — does not count.
#pragma once
#include <stdint.h>

#include "k_ragged_common.hpp"

namespace sicn {

// v_alignbyte_b32: bytes sh .. sh + 3 of the 8 bytes { lo, hi }
SICN_HD inline uint32_t planar_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (sh & 3)));
#endif
}

// v_perm_b32 for the selectors used here: byte i of the result is byte sel[i] of the 8 bytes { lo, hi } (0 .. 3 = lo, 4 .. 7 = hi),
// or zero for selector 0x0c
SICN_HD inline uint32_t planar_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t s = (sel >> (8 * i)) & 255u;
        if (s < 8) r |= (uint32_t)((both >> (8 * s)) & 255u) << (8 * i);
    }
    return r;
#endif
}

// the 4-byte window at address p of a plane: its byte phase and the aligned dwords it lies in
struct PlanarWindow {
    uintptr_t a0;       // the aligned dword that holds the window's first byte
    uint32_t sh;        // p - a0
    bool ld0, ld1;      // which of a0 and a0 + 4 to load: it holds bytes of the window AND overlaps the tensor
};
SICN_HD inline PlanarWindow planar_window(uintptr_t p, uintptr_t lo, uintptr_t hi)
{
    PlanarWindow w;
    w.sh = (uint32_t)p & 3u;
    w.a0 = p - w.sh;
    w.ld0 = w.a0 + 4 > lo && w.a0 < hi;
    w.ld1 = w.sh != 0 && w.a0 + 8 > lo && w.a0 + 4 < hi;
    return w;
}

// byte offset of plane c, row y, column x in an image of planes [h][w]
SICN_HD inline int64_t planar_at(int c, int64_t y, int64_t x, int w, int h) { return ((int64_t)c * h + y) * w + x; }

struct PlanarQuad {
    uint32_t px[4];     // RGBX of pixels ix .. ix + 3
};

// The quad of patch row iy from column ix on (ix may be negative, ix + 3 may pass the row's end) of the image at address im, planes
// [IH][IW]; [lo, hi): the whole tensor.  load(a): the aligned dword at address a.
template <class Load>
SICN_HD inline PlanarQuad planar_quad(uintptr_t im, int IW, int IH, int iy, int ix, uintptr_t lo, uintptr_t hi, Load load)
{
    PlanarQuad q = {{0u, 0u, 0u, 0u}};
    if (iy < 0 || iy >= IH || ix + 3 < 0 || ix >= IW) return q;
    uint32_t pl[3];
    for (int c = 0; c < 3; c++) {
        const PlanarWindow w = planar_window((uintptr_t)((intptr_t)im + planar_at(c, iy, ix, IW, IH)), lo, hi);
        const uint32_t d0 = w.ld0 ? load(w.a0) : 0u, d1 = w.ld1 ? load(w.a0 + 4) : 0u;
        pl[c] = planar_alignbyte(d1, d0, w.sh);
    }
    const uint32_t rg01 = planar_perm(pl[1], pl[0], 0x05010400u);      // R0 G0 R1 G1
    const uint32_t rg23 = planar_perm(pl[1], pl[0], 0x07030602u);      // R2 G2 R3 G3
    q.px[0] = (ix + 0 >= 0 && ix + 0 < IW) ? planar_perm(pl[2], rg01, 0x0c040100u) : 0u;
    q.px[1] = (ix + 1 >= 0 && ix + 1 < IW) ? planar_perm(pl[2], rg01, 0x0c050302u) : 0u;
    q.px[2] = (ix + 2 >= 0 && ix + 2 < IW) ? planar_perm(pl[2], rg23, 0x0c060100u) : 0u;
    q.px[3] = (ix + 3 >= 0 && ix + 3 < IW) ? planar_perm(pl[2], rg23, 0x0c070302u) : 0u;
    return q;
}

// one image of a planar output: the sizes its planes have (the cut) and its byte offset in the output tensor.  A table of its own:
// RaggedRow keeps its layout.
struct PlanarOut {
    int32_t w, h;
    int64_t off;
};

// The deconv's epilogue: output pixel (oy, ox) of the reconstruction is stored iff it lies inside the cut, one byte per plane at
// planar_at(c, oy, ox, w, h).
SICN_HD inline bool planar_stored(int oy, int ox, int w, int h) { return oy < h && ox < w; }

}  // namespace sicn
