// The arithmetic of include/sicn_ragged_ctx_roi_move.h: the stream and band capacities of a window of latent rows that moves over a
// mode-4 container, the placement of a position, the layout of the slots in the chain's tensors, and the rows the placement writes
// for the decode kernels and the two cuts.  Plain C++ that also compiles without HIP (tests/cpp/ctx_roi_move_plan_check.cpp runs it
// under the host sanitizers); under hipcc the placement is __host__ __device__, so that k_ctx_roi_place
// (k_ragged_ctx_roi_move.hip) and the host entry points state ONE rule: the pixel axes are roi_move_host.hpp's place_axis, the
// plan of the placed rows is ctx_window_host.hpp's plan_of_sl — called, not restated.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sicn.h"
#include "../../include/sicn_ragged_ctx_roi_move.h"
#include "ctx_window_host.hpp"
#include "roi_move_host.hpp"

namespace sicn_ctx_roi_move {

using sicn_roi_move::AxisPlace;
using sicn_roi_move::place_axis;
using sicn_window::CutRow;
constexpr int UP = SICN_ROI_MOVE_UP_LAYERS;
constexpr int CUT_ROWS = sicn_window::CUT_ROWS;
constexpr uint32_t WPB_DEC = SICN_CTX_ROI_MOVE_STREAMS_PER_ITEM;   // k_ctx_body.hpp's CTX_WPB_DEC (asserted where both are seen)
constexpr uint64_t META_BYTES = 64;                                // a slot's own block of the workspace

// ---- the capacities ----------------------------------------------------------------------------------------------------------
// cap[3] = { max_streams[0], max_streams[1], band_rows_cap }: the exact maxima of the plan over every r0 in [0, H - rh]
inline int capacity(uint32_t W, uint32_t H, uint32_t C, uint32_t S, uint32_t rh, uint32_t cap[3])
{
    if (!cap) return SICN_EINVAL;
    sicn_ragged_ctx_window_image im;
    if (int rc = sicn_ctx_window::plan_of_sl(W, H, C, S, 0, rh, 0, &im)) return rc;      // every limit, before the loop
    uint32_t best[3] = {0, 0, 0};
    for (uint32_t r0 = 0; r0 <= H - rh; r0++) {
        if (int rc = sicn_ctx_window::plan_of_sl(W, H, C, S, r0, rh, 0, &im)) return rc;
        const uint32_t v[3] = {im.end_stream[0] - im.first_stream[0], im.end_stream[1] - im.first_stream[1], im.band_rows};
        for (int k = 0; k < 3; k++)
            if (v[k] > best[k]) best[k] = v[k];
    }
    cap[0] = best[0]; cap[1] = best[1]; cap[2] = best[2];
    return SICN_OK;
}

// ---- the tables --------------------------------------------------------------------------------------------------------------
// One row per slot, constant, uploaded once: what the placement and the kernels need of the slot and of its image.
struct SlotRow {
    uint64_t band_off, lat_off, recon_off, roi_off, meta_off;
    uint32_t image, first_item[2], max_streams[2], band_rows_cap, lat_first_item, pix_first_item;
    int32_t w, h, cw_cap, rh_cap, image_w, image_h, lat_w, lat_h;
    uint32_t lat_c, S;
};
// One row per slot, written by the placement: the streams of both sets the slot selects in this call and where they land (the
// CtxWinRow of k_ragged_ctx.hip without the first items, which are constant here).
struct MoveRow {
    uint64_t lat_bias;                  // band_off - band_row0 * W * C, modulo 2^64: added to the band tensor's address
    uint32_t first[2], end[2];          // per set, in the set's own numbering
    uint32_t symbols;                   // what the selected streams hold
    uint32_t flags;
};
struct Placement {
    MoveRow win;
    CutRow lat_cut, pix_cut;            // band -> window latent, reconstruction -> ROI pixels
    AxisPlace ax, ay;
    uint32_t band_row0, band_rows;
};

// What a position means for a slot: every word the device tables get.  Nothing here can leave the slot's band, window latent,
// reconstruction or pixels, whatever (x0, y0) is: ay.first lies in [0, lat_h - rh_cap], so the plan cannot refuse and its streams
// and band rows are within the capacities, which are the maxima over exactly those rows.
SICN_ROI_HD inline Placement place_slot(const SlotRow &s, int32_t x0, int32_t y0)
{
    const AxisPlace ax = place_axis(x0, s.image_w, s.lat_w, s.w, s.cw_cap, UP), ay = place_axis(y0, s.image_h, s.lat_h, s.h, s.rh_cap, UP);
    sicn_ragged_ctx_window_image im{};
    (void)sicn_ctx_window::plan_of_sl((uint32_t)s.lat_w, (uint32_t)s.lat_h, s.lat_c, s.S, (uint32_t)ay.first, (uint32_t)s.rh_cap, s.band_off, &im);
    const uint64_t row = (uint64_t)s.lat_w * s.lat_c;
    Placement p;
    p.ax = ax; p.ay = ay;
    p.band_row0 = im.band_row0; p.band_rows = im.band_rows;
    p.win.lat_bias = s.band_off - (uint64_t)im.band_row0 * row;
    for (int k = 0; k < 2; k++) { p.win.first[k] = im.first_stream[k]; p.win.end[k] = im.end_stream[k]; }
    p.win.symbols = im.symbols;
    p.win.flags = (ax.moved | ay.moved) ? SICN_ROI_MOVE_CLAMPED : 0u;
    const uint64_t drow = (uint64_t)s.cw_cap * s.lat_c;
    const uint64_t at = s.band_off + ((uint64_t)ay.first - im.band_row0) * row + (uint64_t)ax.first * s.lat_c;
    p.lat_cut = CutRow{(uint32_t)row, (uint32_t)drow, (uint32_t)s.rh_cap, s.lat_first_item, ((row | drow | at | s.lat_off) & 15) == 0 ? 1u : 0u,
                       0u, (int64_t)at, (int64_t)s.lat_off};
    const uint64_t prow = ((uint64_t)s.cw_cap << UP) * 3, qrow = (uint64_t)s.w * 3;
    const uint64_t pat = s.recon_off + (uint64_t)ay.inside * prow + (uint64_t)ax.inside * 3;
    p.pix_cut = CutRow{(uint32_t)prow, (uint32_t)qrow, (uint32_t)s.h, s.pix_first_item, ((prow | qrow | pat | s.roi_off) & 15) == 0 ? 1u : 0u,
                       0u, (int64_t)pat, (int64_t)s.roi_off};
    return p;
}

// the slot of the geometry alone, for the pure-host placement: no offsets but the band's
inline int slot_of(int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, uint32_t lat_c, uint32_t S, int32_t w, int32_t h,
                   uint64_t band_offset, SlotRow *out)
{
    int32_t cap[2];
    if (int rc = sicn_roi_move::capacity(UP, image_w, image_h, lat_w, lat_h, w, h, cap)) return rc;
    sicn_ragged_ctx_window_image im;
    if (int rc = sicn_ctx_window::plan_of_sl((uint32_t)lat_w, (uint32_t)lat_h, lat_c, S, 0, (uint32_t)cap[1], 0, &im)) return rc;
    if (band_offset >= ((uint64_t)1 << 62)) return SICN_EINVAL;
    SlotRow s{};
    s.band_off = band_offset;
    s.w = w; s.h = h; s.cw_cap = cap[0]; s.rh_cap = cap[1];
    s.image_w = image_w; s.image_h = image_h; s.lat_w = lat_w; s.lat_h = lat_h;
    s.lat_c = lat_c; s.S = S;
    *out = s;
    return SICN_OK;
}

inline int place(int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, uint32_t lat_c, uint32_t S, int32_t w, int32_t h, int32_t x0,
                 int32_t y0, uint64_t band_offset, sicn_ragged_ctx_roi_placed *out)
{
    if (!out) return SICN_EINVAL;
    SlotRow s;
    if (int rc = slot_of(image_w, image_h, lat_w, lat_h, lat_c, S, w, h, band_offset, &s)) return rc;
    const Placement p = place_slot(s, x0, y0);
    sicn_ragged_ctx_roi_placed q{};
    q.px = sicn_ragged_roi_placed{p.ax.pos, p.ay.pos, p.ax.first, p.ay.first, s.cw_cap, s.rh_cap, p.ax.inside, p.ay.inside, p.win.flags};
    for (int k = 0; k < 2; k++) { q.first_stream[k] = p.win.first[k]; q.end_stream[k] = p.win.end[k]; }
    q.band_row0 = p.band_row0; q.band_rows = p.band_rows;
    q.symbols = p.win.symbols;
    q.lat_bias = p.win.lat_bias;
    q.cut_offset = (uint64_t)p.lat_cut.src_off;
    *out = q;
    return SICN_OK;
}

// ---- the layout ----------------------------------------------------------------------------------------------------------------
struct Totals {
    uint64_t band = 0, latent = 0, recon = 0, roi = 0, workspace = 0;
    uint64_t items[2] = {0, 0}, lat_items = 0, pix_items = 0;
};

// coder_ws_bytes: the full ctx coder's workspace for the same images (sicn_ragged_ctx_layout's totals[2]), which this header
// cannot compute without the coder's own.  rows_or_null / slots_out_or_null: [n_slots].
inline int layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *wss_or_null, const uint32_t *image_w,
                  const uint32_t *image_h, uint64_t coder_ws_bytes, int n_images, const sicn_ragged_roi_slot *slots, int n_slots,
                  SlotRow *rows_or_null, sicn_ragged_ctx_roi_move_slot *slots_out_or_null, Totals *totals)
{
    if (!lat_w || !lat_h || !image_w || !image_h || !slots || n_images < 1 || n_slots < 1 || lat_c < 1) return SICN_EINVAL;
    if ((coder_ws_bytes & 15) || coder_ws_bytes >= ((uint64_t)1 << 62)) return SICN_EINVAL;
    Totals t;
    t.workspace = coder_ws_bytes;
    for (int k = 0; k < n_slots; k++) {
        const sicn_ragged_roi_slot &q = slots[k];
        if (q.image < 0 || q.image >= n_images) return SICN_EINVAL;
        const uint32_t lw = lat_w[q.image], lh = lat_h[q.image], iw = image_w[q.image], ih = image_h[q.image];
        const uint32_t S = wss_or_null ? wss_or_null[q.image] : (uint32_t)sicn_ctx_window::WSS;
        if (lw < 1 || lh < 1 || lw > (1u << 20) || lh > (1u << 20) || iw > 0x7fffffffu || ih > 0x7fffffffu) return SICN_EINVAL;
        int32_t cap[2];
        if (int rc = sicn_roi_move::capacity(UP, (int32_t)iw, (int32_t)ih, (int32_t)lw, (int32_t)lh, q.w, q.h, cap)) return rc;
        uint32_t sc[3];
        if (int rc = capacity(lw, lh, lat_c, S, (uint32_t)cap[1], sc)) return rc;
        const uint64_t rw = (uint64_t)cap[0] << UP, rh = (uint64_t)cap[1] << UP;
        if ((double)rw * (double)rh * 3.0 >= (double)sicn_window::MAX_IMAGE_BYTES) return SICN_EINVAL;
        const uint64_t it[2] = {((uint64_t)sc[0] + WPB_DEC - 1) / WPB_DEC, ((uint64_t)sc[1] + WPB_DEC - 1) / WPB_DEC};
        SlotRow s{};
        s.band_off = t.band; s.lat_off = t.latent; s.recon_off = t.recon; s.roi_off = t.roi; s.meta_off = t.workspace;
        s.image = (uint32_t)q.image;
        s.first_item[0] = (uint32_t)t.items[0]; s.first_item[1] = (uint32_t)t.items[1];
        s.max_streams[0] = sc[0]; s.max_streams[1] = sc[1]; s.band_rows_cap = sc[2];
        s.lat_first_item = (uint32_t)t.lat_items; s.pix_first_item = (uint32_t)t.pix_items;
        s.w = q.w; s.h = q.h; s.cw_cap = cap[0]; s.rh_cap = cap[1];
        s.image_w = (int32_t)iw; s.image_h = (int32_t)ih; s.lat_w = (int32_t)lw; s.lat_h = (int32_t)lh;
        s.lat_c = lat_c; s.S = S;
        if (rows_or_null) rows_or_null[k] = s;
        if (slots_out_or_null)
            slots_out_or_null[k] = sicn_ragged_ctx_roi_move_slot{s.band_off, s.lat_off, s.recon_off, s.roi_off, s.meta_off, (uint32_t)cap[0],
                                                                 (uint32_t)cap[1], sc[2], {sc[0], sc[1]}, {s.first_item[0], s.first_item[1]},
                                                                 {(uint32_t)it[0], (uint32_t)it[1]}, 0u};
        t.band += sicn_ctx_window::a16((uint64_t)sc[2] * lw * lat_c);
        t.latent += (uint64_t)cap[1] * cap[0] * lat_c;
        t.recon += rw * rh * 3;
        t.roi += (uint64_t)q.h * q.w * 3;
        t.workspace += META_BYTES;
        t.items[0] += it[0];
        t.items[1] += it[1];
        t.lat_items += ((uint64_t)cap[1] + CUT_ROWS - 1) / CUT_ROWS;
        t.pix_items += ((uint64_t)q.h + CUT_ROWS - 1) / CUT_ROWS;
        if (t.items[0] >= (uint64_t)sicn::RAGGED_MAX_ITEMS || t.items[1] >= (uint64_t)sicn::RAGGED_MAX_ITEMS ||
            t.lat_items >= (uint64_t)sicn::RAGGED_MAX_ITEMS || t.pix_items >= (uint64_t)sicn::RAGGED_MAX_ITEMS ||
            t.workspace >= ((uint64_t)1 << 62) || t.band >= ((uint64_t)1 << 62))
            return SICN_EINVAL;
    }
    if (totals) *totals = t;
    return SICN_OK;
}

}  // namespace sicn_ctx_roi_move
