// The arithmetic of include/sicn_ragged_ctx_roi_move.h: the stream and band capacities of a window of latent rows that moves over a
// mode-4 container, the placement of a position, the layout of the slots in the chain's tensors, and the rows the placement writes
// for the decode kernels and the two cuts.  Plain C++ that also compiles without HIP (tests/cpp/ctx_roi_move_plan_check.cpp runs it
// under the host sanitizers); under hipcc the placement is __host__ __device__, so that k_ctx_roi_place
// (k_ragged_ctx_roi_move.hip) and the host entry points state ONE rule.  What a slot is whatever its coder — the SlotGeom, the pixel
// side of a placement, the latent cut, the shared part of the layout — is roi_move_host.hpp's; the plan of the placed rows is
// ctx_window_host.hpp's plan_of_sl: called, not restated.  What stands here is rANS-WC's own: the capacities of both sets and of
// the band, the streams a placement selects, the meta blocks and the decode items.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sicn.h"
#include "../../include/sicn_ragged_ctx_roi_move.h"
#include "ctx_window_host.hpp"
#include "roi_move_host.hpp"

namespace sicn_ctx_roi_move {

using sicn_roi_move::PixelPlace, sicn_roi_move::SlotGeom, sicn_roi_move::UP, sicn_window::CutRow;
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
struct SlotRow : SlotGeom {
    uint64_t meta_off;
    uint32_t first_item[2], max_streams[2], band_rows_cap, S;
};
// One row per slot, written by the placement: the streams of both sets the slot selects in this call and where they land (the
// CtxWinRow of k_ragged_ctx.hip without the first items, which are constant here).
struct MoveRow {
    uint64_t lat_bias;                  // band_off - band_row0 * W * C, modulo 2^64: added to the band tensor's address
    uint32_t first[2], end[2];          // per set, in the set's own numbering
    uint32_t symbols;                   // what the selected streams hold
    uint32_t flags;
};
struct Placement : PixelPlace {
    MoveRow win;
    CutRow lat_cut;                     // band -> window latent
    uint32_t band_row0, band_rows;
};

// What a position means for a slot: every word the device tables get.  Nothing here can leave the slot's band, window latent,
// reconstruction or pixels, whatever (x0, y0) is: ay.first lies in [0, lat_h - rh_cap], so the plan cannot refuse and its streams
// and band rows are within the capacities, which are the maxima over exactly those rows.
SICN_HD inline Placement place_slot(const SlotRow &s, int32_t x0, int32_t y0)
{
    Placement p{sicn_roi_move::place_pixels(s, x0, y0), {}, {}, 0, 0};
    sicn_ragged_ctx_window_image im{};
    (void)sicn_ctx_window::plan_of_sl((uint32_t)s.lat_w, (uint32_t)s.lat_h, s.lat_c, s.S, (uint32_t)p.ay.first, (uint32_t)s.rh_cap, s.band_off, &im);
    const uint64_t row = (uint64_t)s.lat_w * s.lat_c;
    p.band_row0 = im.band_row0; p.band_rows = im.band_rows;
    p.win = MoveRow{s.band_off - (uint64_t)im.band_row0 * row, {im.first_stream[0], im.first_stream[1]}, {im.end_stream[0], im.end_stream[1]},
                    im.symbols, p.flags};
    p.lat_cut = sicn_roi_move::lat_cut_of(s, p.ax, s.band_off + ((uint64_t)p.ay.first - im.band_row0) * row);
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
    *out = SlotRow{};
    static_cast<SlotGeom &>(*out) = SlotGeom{band_offset, 0, 0, 0, 0, 0, 0, w, h, cap[0], cap[1], image_w, image_h, lat_w, lat_h, lat_c};
    out->S = S;
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
struct Totals : sicn_roi_move::GeomTotals {
    uint64_t items[2] = {0, 0};
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
        SlotRow s{};
        if (int rc = sicn_roi_move::slot_geom(lat_w, lat_h, lat_c, image_w, image_h, n_images, slots[k], &t, &s)) return rc;
        s.S = wss_or_null ? wss_or_null[s.image] : (uint32_t)sicn_ctx_window::WSS;
        uint32_t sc[3];
        if (int rc = capacity((uint32_t)s.lat_w, (uint32_t)s.lat_h, lat_c, s.S, (uint32_t)s.rh_cap, sc)) return rc;
        const uint32_t it[2] = {(sc[0] + WPB_DEC - 1) / WPB_DEC, (sc[1] + WPB_DEC - 1) / WPB_DEC};
        s.meta_off = t.workspace;
        for (int set = 0; set < 2; set++) { s.first_item[set] = (uint32_t)t.items[set]; s.max_streams[set] = sc[set]; }
        s.band_rows_cap = sc[2];
        if (rows_or_null) rows_or_null[k] = s;
        if (slots_out_or_null)
            slots_out_or_null[k] = sicn_ragged_ctx_roi_move_slot{s.band_off, s.lat_off, s.recon_off, s.roi_off, s.meta_off, (uint32_t)s.cw_cap,
                                                                 (uint32_t)s.rh_cap, sc[2], {sc[0], sc[1]}, {s.first_item[0], s.first_item[1]},
                                                                 {it[0], it[1]}, 0u};
        t.items[0] += it[0];
        t.items[1] += it[1];
        if (sicn_roi_move::grow(&t, (uint64_t)sc[2] * s.lat_w * lat_c, META_BYTES) || t.items[0] >= (uint64_t)sicn::RAGGED_MAX_ITEMS ||
            t.items[1] >= (uint64_t)sicn::RAGGED_MAX_ITEMS)
            return SICN_EINVAL;
    }
    if (totals) *totals = t;
    return SICN_OK;
}

}  // namespace sicn_ctx_roi_move
