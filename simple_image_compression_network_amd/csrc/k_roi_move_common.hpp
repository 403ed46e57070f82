// What the two moving ROI decodes hold in common on the device (k_ragged_roi_move.hip over rANS-W, k_ragged_ctx_roi_move.hip over
// rANS-WC): the tables that do not depend on the coder, built, released and cut from in ONE place.  Slot and Move are the coder's
// SlotRow and MoveRow (roi_move_host.hpp, ctx_roi_move_host.hpp); nothing else here differs between the two.
#pragma once
#include <vector>

#include "roi_move_host.hpp"
#include "sicn_internal.h"
#include "sicn_weights_io.h"

namespace sicn_roi_move {

// counts[k] work items of slot k -> the grid's table on the device, the slot of every item: ONE load resolves item -> slot.
// *items: the grid.  An empty grid has no table.
inline bool upload_item_slots(const std::vector<uint32_t> &counts, uint32_t **dev, unsigned *items = nullptr)
{
    std::vector<uint32_t> map;
    for (size_t k = 0; k < counts.size(); k++) map.insert(map.end(), (size_t)counts[k], (uint32_t)k);
    if (items) *items = (unsigned)map.size();
    return map.empty() || sicn::upload(map.data(), map.size() * sizeof(uint32_t), dev);
}

template <class Slot, class Move>
struct MoveTables {
    Slot *d_srows = nullptr;                                            // [n_slots] constant: it begins with the shared SlotGeom
    uint32_t *d_lat_item_slot = nullptr, *d_pix_item_slot = nullptr;    // the two cuts' grids, which the capacities fix
    unsigned lat_items = 0, pix_items = 0;
    Move *d_mrows = nullptr;                                            // [n_slots] each, written by the coder's place kernel
    CutRow *d_lat_rows = nullptr, *d_pix_rows = nullptr;

    // The rows the placement writes start as the placement of (0, 0): a cut that runs before any decode stays in bounds.
    bool build(const std::vector<Slot> &srows)
    {
        std::vector<uint32_t> lat_n, pix_n;
        std::vector<Move> mrows;
        std::vector<CutRow> lat_rows, pix_rows;
        for (const Slot &s : srows) {
            lat_n.push_back((uint32_t)((s.rh_cap + CUT_ROWS - 1) / CUT_ROWS));
            pix_n.push_back((uint32_t)((s.h + CUT_ROWS - 1) / CUT_ROWS));
            const auto p = place_slot(s, 0, 0);
            mrows.push_back(p.win);
            lat_rows.push_back(p.lat_cut);
            pix_rows.push_back(p.pix_cut);
        }
        return sicn::upload(srows.data(), srows.size() * sizeof(Slot), &d_srows) && upload_item_slots(lat_n, &d_lat_item_slot, &lat_items) &&
               upload_item_slots(pix_n, &d_pix_item_slot, &pix_items) && sicn::upload(mrows.data(), mrows.size() * sizeof(Move), &d_mrows) &&
               sicn::upload(lat_rows.data(), lat_rows.size() * sizeof(CutRow), &d_lat_rows) &&
               sicn::upload(pix_rows.data(), pix_rows.size() * sizeof(CutRow), &d_pix_rows);
    }

    void release()
    {
        for (void *b : {(void *)d_srows, (void *)d_lat_item_slot, (void *)d_pix_item_slot, (void *)d_mrows, (void *)d_lat_rows, (void *)d_pix_rows})
            if (b) (void)hipFree(b);
    }

    // k_ragged_cut over the rows of the last placement: band -> window latent, or (pixels) reconstruction -> ROI pixels
    int cut(bool pixels, const uint8_t *src, uint8_t *dst, void *hip_stream) const
    {
        if (!src || !dst) return SICN_EINVAL;
        if (int rc = sicn::chip_geom(nullptr)) return rc;
        return pixels ? sicn::ragged_cut_launch(d_pix_rows, d_pix_item_slot, pix_items, src, dst, hip_stream)
                      : sicn::ragged_cut_launch(d_lat_rows, d_lat_item_slot, lat_items, src, dst, hip_stream);
    }
};

// the four words of a placement that both place kernels store: the streams the slot selects now, the two CutRows, the flags word
template <class Placed, class Move>
__device__ __forceinline__ void store_placement(uint32_t slot, const Placed &p, Move *__restrict__ mrows, CutRow *__restrict__ lat_rows,
                                                CutRow *__restrict__ pix_rows, uint32_t *__restrict__ flags)
{
    mrows[slot] = p.win;
    lat_rows[slot] = p.lat_cut;
    pix_rows[slot] = p.pix_cut;
    flags[slot] = p.flags;
}

}  // namespace sicn_roi_move
