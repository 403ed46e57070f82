// The arithmetic of include/sicn_ragged_window.h on the host: the latent window a pixel rectangle needs, the streams and the band
// of a window of latent rows, and the tables of the cut.  Plain C++ without HIP, so that it also compiles into a stand-alone program
// (tests/cpp/window_plan_check.cpp runs it under the host sanitizers).  k_ragged_window.hip wraps these in the extern "C" entry points.
// What a placement on the device needs as well is SICN_HD (k_ragged_common.hpp): the margins, floor_div / ceil_div, the streams of a
// window of rows (streams_of_rows) and the one statement of a CutRow (cut_row); the moving ROI decodes call them, they restate none.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sicn.h"
#include "../../include/sicn_ragged_window.h"
#include "k_ragged_common.hpp"

namespace sicn_window {

constexpr int MAX_UP_LAYERS = 12;
constexpr uint32_t SELF_SCAN_MAX = 2048;             // streams per image of the ragged coder (k_codec_body.hpp)
constexpr int64_t MAX_IMAGE_BYTES = 0x80000000ll;    // one image's tensor stays below this (sicn_ragged_crop_layout)
constexpr int CUT_ROWS = SICN_RAGGED_CROP_ROWS;

constexpr uint64_t a16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

// m' = 2 m + 1, n' = 2 n + 2 per deconv522 layer, from m = n = 0, in closed form
SICN_HD inline int64_t margin_lo(int n_up_layers) { return ((int64_t)1 << n_up_layers) - 1; }
SICN_HD inline int64_t margin_hi(int n_up_layers) { return 2 * (((int64_t)1 << n_up_layers) - 1); }

SICN_HD inline int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0
SICN_HD inline int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

// one axis: pixels [p0, p0 + len) of an image `image` long, reconstructed from `lat` latent positions
inline bool axis(int64_t p0, int64_t len, int64_t image, int64_t lat, int n_up_layers, int64_t lo, int64_t hi, int32_t *first, int32_t *count,
                 int32_t *inside)
{
    const int64_t scale = (int64_t)1 << n_up_layers;
    if (image < 1 || lat < 1 || lat > (1 << 20) || image > lat * scale) return false;
    if (len < 1 || p0 < 0 || p0 > image || len > image - p0) return false;
    int64_t a = floor_div(p0 - lo, scale), b = ceil_div(p0 + len + hi, scale);
    if (a < 0) a = 0;
    if (b > lat) b = lat;
    *first = (int32_t)a;
    *count = (int32_t)(b - a);
    *inside = (int32_t)(p0 - a * scale);
    return true;
}

inline int roi_plan(int n_up_layers, int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, const sicn_ragged_rect *rect,
                    sicn_ragged_roi *out)
{
    if (!rect || !out || n_up_layers < 1 || n_up_layers > MAX_UP_LAYERS) return SICN_EINVAL;
    const int64_t lo = margin_lo(n_up_layers), hi = margin_hi(n_up_layers);
    sicn_ragged_roi r{};
    if (!axis(rect->x0, rect->w, image_w, lat_w, n_up_layers, lo, hi, &r.c0, &r.cw, &r.x)) return SICN_EINVAL;
    if (!axis(rect->y0, rect->h, image_h, lat_h, n_up_layers, lo, hi, &r.r0, &r.rh, &r.y)) return SICN_EINVAL;
    r.margin_lo = (int32_t)lo;
    r.margin_hi = (int32_t)hi;
    *out = r;
    return SICN_OK;
}

inline bool stream_length_ok(uint32_t wss) { return wss >= 1024u && wss <= 16384u && (wss & (wss - 1u)) == 0; }

// a latent the ragged coder takes: at most SELF_SCAN_MAX streams of an admissible length
inline bool latent_ok(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t wss)
{
    if (lat_w < 1 || lat_h < 1 || lat_c < 1 || !stream_length_ok(wss)) return false;
    const uint64_t most = (uint64_t)SELF_SCAN_MAX * wss;                 // <= 2^25: the products of such a latent cannot wrap
    const uint64_t positions = (uint64_t)lat_w * lat_h;
    return positions <= most && positions * lat_c <= most;
}

// The streams [first, end) that hold latent rows [r0, r0 + rh) of `row` bytes each, of a latent of n symbols cut into streams of wss:
// `symbols` is what those streams hold, `lead` the bytes of the first one that come before row r0.
struct RowStreams {
    uint32_t first, end, symbols, lead;
};
SICN_HD inline RowStreams streams_of_rows(uint64_t row, uint64_t n, uint64_t wss, uint64_t r0, uint64_t rh)
{
    const uint64_t first = r0 * row / wss, end = ((r0 + rh) * row + wss - 1) / wss;
    const uint64_t stop = end * wss < n ? end * wss : n;
    return RowStreams{(uint32_t)first, (uint32_t)end, (uint32_t)(stop - first * wss), (uint32_t)(r0 * row - first * wss)};
}

// The band of one image: rows [r0, r0 + rh) of a [lat_h][lat_w][lat_c] latent cut into streams of wss symbols.
inline int band_of(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t wss, uint32_t r0, uint32_t rh, uint64_t band_offset,
                   sicn_ragged_window_image *out)
{
    if (!latent_ok(lat_w, lat_h, lat_c, wss)) return SICN_EINVAL;
    if (rh < 1 || r0 >= lat_h || rh > lat_h - r0) return SICN_EINVAL;
    const uint64_t row = (uint64_t)lat_w * lat_c;
    const RowStreams st = streams_of_rows(row, row * lat_h, wss, r0, rh);
    out->band_offset = band_offset;
    out->band_bytes = st.symbols;
    out->first_stream = st.first;
    out->end_stream = st.end;
    out->lead = st.lead;
    return SICN_OK;
}

// images_or_null: [n_images].  *band_total: bytes of the band tensor; *streams: the selected streams of all images.
inline int window_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *wss_or_null, const uint32_t *r0,
                         const uint32_t *rh, int n_images, sicn_ragged_window_image *images_or_null, uint64_t *band_total, uint64_t *streams)
{
    if (!lat_w || !lat_h || !r0 || !rh || n_images < 1) return SICN_EINVAL;
    uint64_t at = 0, sel = 0;
    for (int i = 0; i < n_images; i++) {
        sicn_ragged_window_image im;
        if (int rc = band_of(lat_w[i], lat_h[i], lat_c, wss_or_null ? wss_or_null[i] : 16384u, r0[i], rh[i], at, &im)) return rc;
        if (images_or_null) images_or_null[i] = im;
        at += a16(im.band_bytes);
        sel += im.end_stream - im.first_stream;
    }
    if (band_total) *band_total = at;
    if (streams) *streams = sel;
    return SICN_OK;
}

// ---- the cut ------------------------------------------------------------------------------------------------------------------
// One row per image, as the kernel loads it.  src_off leads to the RECTANGLE's first byte: the image's offset, y0 rows and x0 pixels.
struct CutRow {
    uint32_t src_row, dst_row, dst_h, first_item, vec, pad;
    int64_t src_off, dst_off;
};
// vec: every row of both sides begins on 16 bytes, so the kernel moves dwordx4
SICN_HD inline CutRow cut_row(uint64_t src_row, uint64_t dst_row, uint32_t dst_h, uint32_t first_item, uint64_t src_off, uint64_t dst_off)
{
    return CutRow{(uint32_t)src_row, (uint32_t)dst_row, dst_h, first_item, ((src_row | dst_row | src_off | dst_off) & 15) == 0 ? 1u : 0u, 0u,
                  (int64_t)src_off, (int64_t)dst_off};
}

// rows_or_null: [n_images]; first_item_or_null: [n_images + 1]; image_off_or_null: [n_images] the source images' own offsets.
// totals: { bytes of the source tensor (the furthest byte a source image reaches), bytes of the destination tensor }.
inline int cut_plan(const int32_t *src_w, const int32_t *src_h, const sicn_ragged_rect *rects, int channels, const uint64_t *src_offset_or_null,
                    int n_images, CutRow *rows_or_null, int64_t *first_item_or_null, int64_t *image_off_or_null, int64_t totals[2])
{
    if (!src_w || !src_h || !rects || n_images < 1 || channels < 1) return SICN_EINVAL;
    int64_t so = 0, dof = 0, reach = 0, item = 0;
    for (int i = 0; i < n_images; i++) {
        const sicn_ragged_rect &q = rects[i];
        if (src_w[i] < 1 || src_h[i] < 1 || src_w[i] > (1 << 20) || src_h[i] > (1 << 20)) return SICN_EINVAL;
        if (q.w < 1 || q.h < 1 || q.x0 < 0 || q.y0 < 0 || q.x0 > src_w[i] || q.w > src_w[i] - q.x0 || q.y0 > src_h[i] || q.h > src_h[i] - q.y0)
            return SICN_EINVAL;
        if ((double)src_h[i] * src_w[i] * channels >= (double)MAX_IMAGE_BYTES) return SICN_EINVAL;   // before the 64-bit product can overflow
        const int64_t srow = (int64_t)src_w[i] * channels, drow = (int64_t)q.w * channels;
        if (src_offset_or_null) {
            if (src_offset_or_null[i] >= ((uint64_t)1 << 62)) return SICN_EINVAL;
            so = (int64_t)src_offset_or_null[i];
        }
        const int64_t at = so + (int64_t)q.y0 * srow + (int64_t)q.x0 * channels;
        if (rows_or_null) rows_or_null[i] = cut_row((uint64_t)srow, (uint64_t)drow, (uint32_t)q.h, (uint32_t)item, (uint64_t)at, (uint64_t)dof);
        if (first_item_or_null) first_item_or_null[i] = item;
        if (image_off_or_null) image_off_or_null[i] = so;
        item += (q.h + CUT_ROWS - 1) / CUT_ROWS;
        if (item >= sicn::RAGGED_MAX_ITEMS) return SICN_EINVAL;
        so += srow * src_h[i];
        if (so > reach) reach = so;
        dof += drow * q.h;
    }
    if (first_item_or_null) first_item_or_null[n_images] = item;
    if (totals) {
        totals[0] = reach;
        totals[1] = dof;
    }
    return SICN_OK;
}

}  // namespace sicn_window
