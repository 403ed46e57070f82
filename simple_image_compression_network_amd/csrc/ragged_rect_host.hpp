// The rectangle epilogue of the packed deconv N -> 3 of a ragged net (include/sicn_ragged_rect.h): which pixels of a reconstruction
// the lane stores, where in the image's own 3 h w bytes, and which tiles have nothing to store.  Everything here is SICN_HD
// (k_ragged_common.hpp): k_rgb_deconv_ragged_rect and k_rgb_deconv_ragged_planar_rect of k_ragged_rgb.hip evaluate it on the device,
// k_ragged.hip counts live tiles with it and tests/cpp/ragged_rect_check.cpp replays it on the host over byte arrays of exactly
// 3 h w bytes.
//
// The rectangle is (x0, y0, w, h): w and h are the creation's, 1 <= w, h <= 2^21; the origin (x0, y0) is ANY pair of int32 — it may
// come from device memory when the kernel runs.  Output pixel (oy, ox) of the R_h x R_w reconstruction has the in-rectangle
// coordinates (oy - y0, ox - x0).  They are taken in uint32: 0 <= oy, ox < 2^22, so the true difference lies in (-2^31, 2^31 + 2^22)
// and its residue mod 2^32 is below h (w) exactly where the difference itself is in [0, h) ([0, w)).  The address is formed from
// these coordinates alone, so a store lies inside the image's own 3 h w bytes whatever the origin is; a rectangle that reaches outside
// the reconstruction leaves the bytes out there unwritten.  There is no clamp.
#pragma once
#include <stdint.h>

#include "k_ragged_common.hpp"
#include "ragged_planar_host.hpp"

namespace sicn {

constexpr int RECT_TILE_OUT = 32;      // a tile of 16 x 16 input positions is 32 x 32 output pixels

// coordinate o >= 0 of the reconstruction relative to the origin: the residue mod 2^32 of o - origin
SICN_HD inline uint32_t rect_rel(int o, int32_t origin) { return (uint32_t)o - (uint32_t)origin; }

// Is output pixel (oy, ox) stored?  It is one of the reconstruction's R_h x R_w (the tile computes lanes beyond the image's edge from
// padding; they are never stored) and it lies inside the rectangle.
SICN_HD inline bool rect_stored(int oy, int ox, int R_w, int R_h, int32_t x0, int32_t y0, int w, int h)
{
    return oy < R_h && ox < R_w && rect_rel(oy, y0) < (uint32_t)h && rect_rel(ox, x0) < (uint32_t)w;
}

// byte offset of channel c of in-rectangle pixel (ry, rx) in the image's own bytes: [h][w][3], or planes [3][h][w]
template <bool PLANAR>
SICN_HD inline int64_t rect_at(int c, uint32_t ry, uint32_t rx, int w, int h)
{
    if (PLANAR) return planar_at(c, (int64_t)ry, (int64_t)rx, w, h);
    return ((int64_t)ry * w + (int64_t)rx) * 3 + c;
}

// Does the tile whose first input position is (ty0, tx0) — output rows [2 ty0, 2 ty0 + 32), columns alike — meet the rectangle?
// 64-bit: x0 + w passes int32 for origins near its end.
SICN_HD inline bool rect_tile_live(int ty0, int tx0, int32_t x0, int32_t y0, int w, int h)
{
    const int64_t ya = 2 * (int64_t)ty0, xa = 2 * (int64_t)tx0;
    return ya < (int64_t)y0 + h && (int64_t)y0 < ya + RECT_TILE_OUT && xa < (int64_t)x0 + w && (int64_t)x0 < xa + RECT_TILE_OUT;
}

#ifdef __HIPCC__
// k_ragged_rgb.hip: the deconv with the rectangle epilogue.  `out` as [h][w][3] or, planar, [3][h][w] per image at the sizes and offsets
// of `cuts`; origins: device int32 [n_images][2], the rectangles' corners (x0, y0), read when the kernel runs.  The other arguments
// are launch_ragged_rgb_deconv_planar's (sicn_internal.h).
hipError_t launch_ragged_rgb_deconv_rect(bool planar, const uint8_t *in, uint8_t *out, const int8_t *wimg, const int8_t *bias,
                                         const RaggedRow *rows, const uint32_t *tile_image, const PlanarOut *cuts, const int32_t *origins,
                                         int cin, unsigned items, uint32_t floor2, hipStream_t stream);
#endif

}  // namespace sicn
