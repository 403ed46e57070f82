// The arithmetic of include/sicn_ragged_roi_move.h: the capacity of a slot's latent window, the placement of a position, the layout
// of the slots in the chain's tensors, and the rows the placement writes for the window decoder and the two cuts.  Plain C++ that
// also compiles without HIP (tests/cpp/roi_move_plan_check.cpp runs it under the host sanitizers); under hipcc the placement is
// __host__ __device__ (SICN_HD), so that k_roi_place (k_ragged_roi_move.hip) and the host entry points state ONE rule.
// What a slot is whatever coder made its containers stands here ONCE, for ctx_roi_move_host.hpp too: the SlotGeom every SlotRow
// begins with, the pixel side of a placement (place_pixels), the latent cut (lat_cut_of) and the shared part of the layout
// (slot_geom, grow).  What is rANS-W's own: the streams a placed window selects, by window_host.hpp's streams_of_rows.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sicn.h"
#include "../../include/sicn_ragged_roi_move.h"
#include "window_host.hpp"

namespace sicn_roi_move {

using sicn_window::CutRow, sicn_window::ceil_div, sicn_window::floor_div, sicn_window::margin_hi, sicn_window::margin_lo;
constexpr int UP = SICN_ROI_MOVE_UP_LAYERS;
constexpr int CUT_ROWS = sicn_window::CUT_ROWS;

// one axis of a slot: a rectangle side `len` in an image side `image` over `lat` latent positions
inline bool axis_ok(int64_t image, int64_t lat, int64_t len, int up)
{
    if (up < 1 || up > sicn_window::MAX_UP_LAYERS) return false;
    if (image < 1 || lat < 1 || lat > (1 << 20) || image > lat * ((int64_t)1 << up)) return false;
    return len >= 1 && len <= image;
}

// the largest unclipped window count over the positions [0, image - len], which has the period 2^up; then clipped to the latent
inline int32_t axis_capacity(int64_t image, int64_t lat, int64_t len, int up)
{
    const int64_t scale = (int64_t)1 << up, lo = margin_lo(up), hi = margin_hi(up);
    int64_t last = image - len, best = 0;
    if (last > scale - 1) last = scale - 1;
    for (int64_t p = 0; p <= last; p++) {
        const int64_t c = ceil_div(p + len + hi, scale) - floor_div(p - lo, scale);
        if (c > best) best = c;
    }
    return (int32_t)(best < lat ? best : lat);
}

struct AxisPlace {
    int32_t pos, first, inside;     // the clamped position, the window's first latent position, the position inside the window
    uint32_t moved;
};

// steps 1 .. 4 of the header's placement rule on one axis; cap = axis_capacity of the same axis
SICN_HD inline AxisPlace place_axis(int64_t p, int64_t image, int64_t lat, int64_t len, int64_t cap, int up)
{
    const int64_t scale = (int64_t)1 << up, last = image - len;
    const int64_t pc = p < 0 ? 0 : p > last ? last : p;
    int64_t a = floor_div(pc - margin_lo(up), scale);       // sicn_ragged_roi_plan's first position
    if (a < 0) a = 0;
    if (a > lat - cap) a = lat - cap;
    return AxisPlace{(int32_t)pc, (int32_t)a, (int32_t)(pc - a * scale), pc != p ? 1u : 0u};
}

inline int capacity(int up, int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, int32_t w, int32_t h, int32_t cap[2])
{
    if (!cap || !axis_ok(image_w, lat_w, w, up) || !axis_ok(image_h, lat_h, h, up)) return SICN_EINVAL;
    cap[0] = axis_capacity(image_w, lat_w, w, up);
    cap[1] = axis_capacity(image_h, lat_h, h, up);
    return SICN_OK;
}

inline int place(int up, int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, int32_t w, int32_t h, int32_t x0, int32_t y0,
                 sicn_ragged_roi_placed *out)
{
    int32_t cap[2];
    if (!out) return SICN_EINVAL;
    if (int rc = capacity(up, image_w, image_h, lat_w, lat_h, w, h, cap)) return rc;
    const AxisPlace ax = place_axis(x0, image_w, lat_w, w, cap[0], up), ay = place_axis(y0, image_h, lat_h, h, cap[1], up);
    *out = sicn_ragged_roi_placed{ax.pos, ay.pos, ax.first, ay.first, cap[0], cap[1], ax.inside, ay.inside,
                                  (ax.moved | ay.moved) ? SICN_ROI_MOVE_CLAMPED : 0u};
    return SICN_OK;
}

// ---- the tables --------------------------------------------------------------------------------------------------------------
// What a slot is whatever coder made its containers: its size and pixel capacities, its image's geometry, its offsets in the four
// tensors both chains have and its first items in the two cuts' grids.  Each coder's SlotRow begins with it.
struct SlotGeom {
    uint64_t band_off, lat_off, recon_off, roi_off;
    uint32_t image, lat_first_item, pix_first_item;
    int32_t w, h, cw_cap, rh_cap, image_w, image_h, lat_w, lat_h;
    uint32_t lat_c;
};
// One row per slot, constant, uploaded once: what the placement and the kernels need of the slot and of its image.
struct SlotRow : SlotGeom {
    uint64_t ws_off;
    uint32_t first_item, max_streams, wss, n;
};
// One row per slot, written by the placement: the streams the slot selects in this call and where they land (the WinRow of
// k_ragged_window.hip without the first item, which is constant here).
struct MoveRow {
    uint64_t lat_bias;                  // band_off - first_stream * wss, modulo 2^64: added to the band tensor's address
    uint32_t first_stream, end_stream;  // in the image's own numbering
    uint32_t symbols;                   // what the selected streams hold
    uint32_t flags;
};
// The pixel side of a placement, which no coder changes: the two axes, the flags word and the cut reconstruction -> ROI pixels.
struct PixelPlace {
    AxisPlace ax, ay;
    uint32_t flags;
    CutRow pix_cut;
};
struct Placement : PixelPlace {
    MoveRow win;
    CutRow lat_cut;                     // band -> window latent
};

SICN_HD inline PixelPlace place_pixels(const SlotGeom &s, int32_t x0, int32_t y0)
{
    const AxisPlace ax = place_axis(x0, s.image_w, s.lat_w, s.w, s.cw_cap, UP), ay = place_axis(y0, s.image_h, s.lat_h, s.h, s.rh_cap, UP);
    const uint64_t prow = ((uint64_t)s.cw_cap << UP) * 3;
    return PixelPlace{ax, ay, (ax.moved | ay.moved) ? SICN_ROI_MOVE_CLAMPED : 0u,
                      sicn_window::cut_row(prow, (uint64_t)s.w * 3, (uint32_t)s.h, s.pix_first_item,
                                           s.recon_off + (uint64_t)ay.inside * prow + (uint64_t)ax.inside * 3, s.roi_off)};
}

// the latent cut of a placement; band_row: where latent row ay.first begins in the band tensor
SICN_HD inline CutRow lat_cut_of(const SlotGeom &s, const AxisPlace &ax, uint64_t band_row)
{
    return sicn_window::cut_row((uint64_t)s.lat_w * s.lat_c, (uint64_t)s.cw_cap * s.lat_c, (uint32_t)s.rh_cap, s.lat_first_item,
                                band_row + (uint64_t)ax.first * s.lat_c, s.lat_off);
}

// What a position means for a slot: every word the device tables get.  Nothing here can leave the slot's band, window latent,
// reconstruction or pixels, whatever (x0, y0) is.
SICN_HD inline Placement place_slot(const SlotRow &s, int32_t x0, int32_t y0)
{
    Placement p{place_pixels(s, x0, y0), {}, {}};
    const sicn_window::RowStreams st =
        sicn_window::streams_of_rows((uint64_t)s.lat_w * s.lat_c, s.n, s.wss, (uint64_t)p.ay.first, (uint64_t)s.rh_cap);
    p.win = MoveRow{s.band_off - (uint64_t)st.first * s.wss, st.first, st.end, st.symbols, p.flags};
    p.lat_cut = lat_cut_of(s, p.ax, s.band_off + st.lead);
    return p;
}

// ---- the layout ----------------------------------------------------------------------------------------------------------------
struct GeomTotals {
    uint64_t band = 0, latent = 0, recon = 0, roi = 0, workspace = 0, lat_items = 0, pix_items = 0;
};
struct Totals : GeomTotals {
    uint64_t items = 0;
};

// The shared part of one slot's layout: the slot against its image, the pixel capacities, the size refusal; *g gets the geometry with
// the offsets and first cut items *t has reached, and *t moves on by what the slot takes of the window latent, the reconstruction,
// the ROI pixels and the two cuts' grids.  The band and the workspace are the coder's to add: grow().
inline int slot_geom(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *image_w, const uint32_t *image_h, int n_images,
                     const sicn_ragged_roi_slot &q, GeomTotals *t, SlotGeom *g)
{
    if (q.image < 0 || q.image >= n_images) return SICN_EINVAL;
    const uint32_t lw = lat_w[q.image], lh = lat_h[q.image], iw = image_w[q.image], ih = image_h[q.image];
    if (lw < 1 || lh < 1 || iw > 0x7fffffffu || ih > 0x7fffffffu) return SICN_EINVAL;
    int32_t cap[2];
    if (int rc = capacity(UP, (int32_t)iw, (int32_t)ih, (int32_t)lw, (int32_t)lh, q.w, q.h, cap)) return rc;
    const uint64_t rw = (uint64_t)cap[0] << UP, rh = (uint64_t)cap[1] << UP;
    if ((double)rw * (double)rh * 3.0 >= (double)sicn_window::MAX_IMAGE_BYTES) return SICN_EINVAL;
    *g = SlotGeom{t->band, t->latent, t->recon, t->roi, (uint32_t)q.image, (uint32_t)t->lat_items, (uint32_t)t->pix_items, q.w, q.h, cap[0], cap[1],
                  (int32_t)iw, (int32_t)ih, (int32_t)lw, (int32_t)lh, lat_c};
    t->latent += (uint64_t)cap[1] * cap[0] * lat_c;
    t->recon += rw * rh * 3;
    t->roi += (uint64_t)q.h * q.w * 3;
    t->lat_items += ((uint64_t)cap[1] + CUT_ROWS - 1) / CUT_ROWS;
    t->pix_items += ((uint64_t)q.h + CUT_ROWS - 1) / CUT_ROWS;
    return t->lat_items >= (uint64_t)sicn::RAGGED_MAX_ITEMS || t->pix_items >= (uint64_t)sicn::RAGGED_MAX_ITEMS ? SICN_EINVAL : SICN_OK;
}

// the slot's band and workspace block, and the limits of both tensors
inline int grow(GeomTotals *t, uint64_t band_bytes, uint64_t ws_bytes)
{
    t->band += sicn_window::a16(band_bytes);
    t->workspace += ws_bytes;
    return t->workspace >= ((uint64_t)1 << 62) || t->band >= ((uint64_t)1 << 62) ? SICN_EINVAL : SICN_OK;
}

// image_ws_bytes: [n_images] the bytes of each image's workspace block in the full coder (sicn_ragged_codec_layout), which this
// header cannot compute without the coder's own.  rows_or_null / slots_out_or_null: [n_slots].
inline int layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *wss_or_null, const uint32_t *image_w,
                  const uint32_t *image_h, const uint64_t *image_ws_bytes, int n_images, const sicn_ragged_roi_slot *slots, int n_slots,
                  SlotRow *rows_or_null, sicn_ragged_roi_move_slot *slots_out_or_null, Totals *totals)
{
    if (!lat_w || !lat_h || !image_w || !image_h || !image_ws_bytes || !slots || n_images < 1 || n_slots < 1 || lat_c < 1) return SICN_EINVAL;
    Totals t;
    for (int k = 0; k < n_slots; k++) {
        SlotRow s{};
        if (int rc = slot_geom(lat_w, lat_h, lat_c, image_w, image_h, n_images, slots[k], &t, &s)) return rc;
        const uint32_t wss = wss_or_null ? wss_or_null[s.image] : 16384u;
        if (!sicn_window::latent_ok((uint32_t)s.lat_w, (uint32_t)s.lat_h, lat_c, wss) || (image_ws_bytes[s.image] & 15)) return SICN_EINVAL;
        // one stream more than rh_cap rows from row 0 need: a window may begin inside a stream
        const uint64_t row = (uint64_t)s.lat_w * lat_c, n = row * s.lat_h;
        const uint32_t all = sicn_window::streams_of_rows(row, n, wss, 0, (uint64_t)s.lat_h).end;
        const uint32_t most = sicn_window::streams_of_rows(row, n, wss, 0, (uint64_t)s.rh_cap).end + 1;
        s.ws_off = t.workspace; s.first_item = (uint32_t)t.items; s.max_streams = most < all ? most : all;
        s.wss = wss; s.n = (uint32_t)n;
        if (rows_or_null) rows_or_null[k] = s;
        if (slots_out_or_null)
            slots_out_or_null[k] = sicn_ragged_roi_move_slot{s.band_off, s.lat_off, s.recon_off, s.roi_off, s.ws_off, (uint32_t)s.cw_cap,
                                                             (uint32_t)s.rh_cap, s.max_streams, s.first_item};
        t.items += s.max_streams;
        if (grow(&t, (uint64_t)s.max_streams * wss, image_ws_bytes[s.image]) || t.items >= (uint64_t)sicn::RAGGED_MAX_ITEMS) return SICN_EINVAL;
    }
    if (totals) *totals = t;
    return SICN_OK;
}

}  // namespace sicn_roi_move
