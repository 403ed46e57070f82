// What the two moving ROI decodes hold in common on the device (k_ragged_roi_move.hip over rANS-W, k_ragged_ctx_roi_move.hip over
// rANS-WC): the tables that do not depend on the coder, built, owned and cut from in ONE place.  Slot and Move are the coder's
// SlotRow and MoveRow (roi_move_host.hpp, ctx_roi_move_host.hpp); nothing else here differs between the two.
#pragma once
#include <vector>

#include "device_table.hpp"
#include "roi_move_host.hpp"
#include "sicn_internal.h"

namespace sicn_roi_move {

template <class Slot, class Move>
struct MoveTables {
    sicn::DeviceTable<Slot> d_srows;                                    // [n_slots] constant: it begins with the shared SlotGeom
    sicn::DeviceTable<uint32_t> d_lat_item_slot, d_pix_item_slot;       // the two cuts' grids, which the capacities fix
    unsigned lat_items = 0, pix_items = 0;
    // [n_slots] each, written by the coder's place kernel on every decode: mutable, because a decode takes the object as const — it
    // changes nothing on the host, and what the device holds is the last placement's by contract
    mutable sicn::DeviceTable<Move> d_mrows;
    mutable sicn::DeviceTable<CutRow> d_lat_rows, d_pix_rows;
    // [n_slots][2]: the placed rectangle's corner (x, y) inside its window reconstruction — the origins a window net made with
    // rectangles reads in place of the pixel cut (include/sicn_ragged_rect.h)
    mutable sicn::DeviceTable<int32_t> d_origins;

    // The rows the placement writes start as the placement of (0, 0): a cut that runs before any decode stays in bounds.
    bool build(const std::vector<Slot> &srows)
    {
        sicn::ItemMap lat_map, pix_map;
        std::vector<Move> mrows;
        std::vector<CutRow> lat_rows, pix_rows;
        std::vector<int32_t> origins;
        for (size_t k = 0; k < srows.size(); k++) {
            const Slot &s = srows[k];
            lat_map.add((uint32_t)((s.rh_cap + CUT_ROWS - 1) / CUT_ROWS), (uint32_t)k);
            pix_map.add((uint32_t)((s.h + CUT_ROWS - 1) / CUT_ROWS), (uint32_t)k);
            const auto p = place_slot(s, 0, 0);
            mrows.push_back(p.win);
            lat_rows.push_back(p.lat_cut);
            pix_rows.push_back(p.pix_cut);
            origins.push_back(p.ax.inside);
            origins.push_back(p.ay.inside);
        }
        lat_items = (unsigned)lat_map.size();
        pix_items = (unsigned)pix_map.size();
        return d_srows.upload(srows) && lat_map.upload(d_lat_item_slot) && pix_map.upload(d_pix_item_slot) && d_mrows.upload(mrows) &&
               d_lat_rows.upload(lat_rows) && d_pix_rows.upload(pix_rows) && d_origins.upload(origins);
    }

    // k_ragged_cut over the rows of the last placement: band -> window latent, or (pixels) reconstruction -> ROI pixels
    int cut(bool pixels, const uint8_t *src, uint8_t *dst, void *hip_stream) const
    {
        if (!src || !dst) return SICN_EINVAL;
        if (int rc = sicn::chip_geom(nullptr)) return rc;
        return pixels ? sicn::ragged_cut_launch(d_pix_rows.get(), d_pix_item_slot.get(), pix_items, src, dst, hip_stream)
                      : sicn::ragged_cut_launch(d_lat_rows.get(), d_lat_item_slot.get(), lat_items, src, dst, hip_stream);
    }
};

// the five words of a placement that both place kernels store: the streams the slot selects now, the two CutRows, the flags word and
// the corner inside the window reconstruction (origins: int32 [n_slots][2], 8-byte aligned)
template <class Placed, class Move>
__device__ __forceinline__ void store_placement(uint32_t slot, const Placed &p, Move *__restrict__ mrows, CutRow *__restrict__ lat_rows,
                                                CutRow *__restrict__ pix_rows, uint32_t *__restrict__ flags, int32_t *__restrict__ origins)
{
    reinterpret_cast<int2 *>(origins)[slot] = int2{p.ax.inside, p.ay.inside};
    mrows[slot] = p.win;
    lat_rows[slot] = p.lat_cut;
    pix_rows[slot] = p.pix_cut;
    flags[slot] = p.flags;
}

}  // namespace sicn_roi_move
