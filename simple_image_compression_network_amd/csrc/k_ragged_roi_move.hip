// Moving ROI decode (include/sicn_ragged_roi_move.h): the window decoder of k_ragged_window.hip over SLOTS whose rectangles are
// placed on the device, from positions read out of device memory on every call.  A translation unit of its own: the kernels of
// k_ragged_window.hip, k_ragged_codec.hip and sicn_codec.hip keep their code as it is.  The two cuts are k_ragged_window.hip's
// k_ragged_cut itself (sicn::ragged_cut_launch) over rows this file writes.
//
// Tables.  What no coder changes is k_roi_move_common.hpp's MoveTables, shared with k_ragged_ctx_roi_move.hip: srows[slot] (SlotRow
// of roi_move_host.hpp: the shared SlotGeom, then the slot's workspace block, first decode item, max_streams and its image's stream
// length and symbols), the two cuts' item -> slot maps, and the rows k_roi_place writes on the stream, one thread per slot, from
// place_slot() — the function the host entry points call too: mrows[slot] (MoveRow, the streams [first_stream, end_stream) the slot
// selects now and where they land in its band), lat_rows[slot], pix_rows[slot], and the caller's flags[slot].  This file's own:
//   item_slot[item]  : the slot of a work item of the decode grid (sum of max_streams) — ONE load resolves item -> slot
//   rows[image]      : the CODER's CoderRow table
// k_roi_move_decode: slot -> image is one more wave-uniform load; a surplus item (its stream >= end_stream) returns before it reads
// or writes anything else; otherwise ransw_decode_body runs unchanged on the slot's OWN workspace block with the stream's real
// index, as in k_ragged_decode_window.  k_roi_move_finish: one workgroup per slot, dec_finish_window_body, one status pair per slot.
#include <new>
#include <vector>

#include "../../include/sicn_ragged_roi_move.h"
#include "k_codec_body.hpp"
#include "../../include/sicn_ragged_rect.h"
#include "k_roi_move_common.hpp"

namespace {

using sicn_roi_move::MoveRow;
using sicn_roi_move::SlotRow;
using sicn_window::CutRow;

__global__ __launch_bounds__(64) void k_roi_place(const int32_t *__restrict__ xy, const SlotRow *__restrict__ srows, uint32_t n_slots,
                                                  MoveRow *__restrict__ mrows, CutRow *__restrict__ lat_rows, CutRow *__restrict__ pix_rows,
                                                  uint32_t *__restrict__ flags, int32_t *__restrict__ origins)
{
    const uint32_t slot = blockIdx.x * 64u + threadIdx.x;
    if (slot >= n_slots) return;
    sicn_roi_move::store_placement(slot, sicn_roi_move::place_slot(srows[slot], xy[2 * (size_t)slot], xy[2 * (size_t)slot + 1]), mrows, lat_rows,
                                   pix_rows, flags, origins);
}

// the slot's image as the stage bodies see it: the coder's row with the slot's own workspace block
__device__ __forceinline__ CoderRow slot_image_row(const CoderRow *__restrict__ rows, const SlotRow *__restrict__ s, uint32_t img)
{
    CoderRow r = load_row(rows, img);
    r.ws_off = uni((uint64_t)s->ws_off);
    return r;
}

template <bool BIGTAB>
__global__ __launch_bounds__(64) void k_roi_move_decode(const uint8_t *__restrict__ containers, const uint32_t *__restrict__ valid,
                                                        uint8_t *__restrict__ band, uint8_t *__restrict__ workspace,
                                                        const CoderRow *__restrict__ rows, const SlotRow *__restrict__ srows,
                                                        const MoveRow *__restrict__ mrows, const uint32_t *__restrict__ item_slot)
{
    const uint32_t slot = uni(item_slot[blockIdx.x]);
    const SlotRow *s = srows + slot;
    const MoveRow *m = mrows + slot;
    const uint32_t st = blockIdx.x - uni(s->first_item) + uni(m->first_stream);
    if (st >= uni(m->end_stream)) return;                    // the capacity's surplus over this position's selection
    const uint32_t img = uni(s->image);
    DecImage im = dec_image(slot_image_row(rows, s, img), containers, valid, band, nullptr, workspace, img);
    im.lat = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(band) + uni((uint64_t)m->lat_bias));
    ransw_decode_body<BIGTAB>(im, st, 1);
}

__global__ __launch_bounds__(256) void k_roi_move_finish(const uint8_t *__restrict__ containers, const uint32_t *__restrict__ valid,
                                                         uint32_t *__restrict__ status, uint8_t *__restrict__ workspace,
                                                         const CoderRow *__restrict__ rows, const SlotRow *__restrict__ srows,
                                                         const MoveRow *__restrict__ mrows)
{
    const uint32_t slot = blockIdx.x;
    const SlotRow *s = srows + slot;
    const MoveRow *m = mrows + slot;
    const uint32_t img = uni(s->image);
    DecImage im = dec_image(slot_image_row(rows, s, img), containers, valid, nullptr, status, workspace, img);
    im.status = status + 2 * (size_t)slot;                   // one status pair per SLOT; `valid` stays the image's
    dec_finish_window_body(im, uni(m->first_stream), uni(m->end_stream), uni(m->symbols));
}

// the full coder's workspace block of every image, from the coder's own rows
int image_workspace_bytes(const CoderRow *rows, int n_images, uint64_t ws_total, std::vector<uint64_t> *out)
{
    out->resize((size_t)n_images);
    for (int i = 0; i < n_images; i++) {
        const uint64_t next = i + 1 < n_images ? rows[i + 1].ws_off : ws_total;
        if (next < rows[i].ws_off) return SICN_EINVAL;
        (*out)[(size_t)i] = next - rows[i].ws_off;
    }
    return SICN_OK;
}

}  // namespace

// ---- capacity, placement, layout: pure host ------------------------------------------------------------------------------------
extern "C" int sicn_ragged_roi_move_capacity(int n_up_layers, int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, int32_t w,
                                             int32_t h, int32_t cap[2])
{
    return sicn_roi_move::capacity(n_up_layers, image_w, image_h, lat_w, lat_h, w, h, cap);
}

extern "C" int sicn_ragged_roi_move_place(int n_up_layers, int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, int32_t w, int32_t h,
                                          int32_t x0, int32_t y0, sicn_ragged_roi_placed *out)
{
    return sicn_roi_move::place(n_up_layers, image_w, image_h, lat_w, lat_h, w, h, x0, y0, out);
}

extern "C" int sicn_ragged_roi_move_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                                           const uint32_t *image_w, const uint32_t *image_h, int n_images, const sicn_ragged_roi_slot *slots,
                                           int n_slots, sicn_ragged_roi_move_slot *slots_out_or_null, uint64_t totals[6])
{
    if (!image_w || !image_h || !slots || n_slots < 1 || n_images < 1) return SICN_EINVAL;
    try {
        std::vector<sicn_ragged_codec_image> images((size_t)n_images);
        std::vector<uint64_t> ws((size_t)n_images);
        uint64_t coder[3] = {0, 0, 0};
        if (int rc = sicn_ragged_codec_layout(lat_w, lat_h, lat_c, stream_symbols_or_null, n_images, images.data(), coder)) return rc;
        for (int i = 0; i < n_images; i++)
            ws[(size_t)i] = (i + 1 < n_images ? images[(size_t)i + 1].workspace_offset : coder[2]) - images[(size_t)i].workspace_offset;
        sicn_roi_move::Totals t;
        if (int rc = sicn_roi_move::layout(lat_w, lat_h, lat_c, stream_symbols_or_null, image_w, image_h, ws.data(), n_images, slots, n_slots,
                                           nullptr, slots_out_or_null, &t))
            return rc;
        if (totals) {
            totals[0] = t.band; totals[1] = t.latent; totals[2] = t.recon; totals[3] = t.roi; totals[4] = t.workspace; totals[5] = t.items;
        }
    } catch (const std::bad_alloc &) { return SICN_ENOMEM; }
    return SICN_OK;
}

// ---- the object ------------------------------------------------------------------------------------------------------------------
struct sicn_ragged_roi_move {
    int n_slots = 0;
    bool bigtab = false;                    // the decode form, chosen once from the capacity
    sicn_roi_move::Totals totals;
    const CoderRow *d_rows = nullptr;       // the coder's
    sicn::DeviceTable<uint32_t> d_item_slot;
    sicn_roi_move::MoveTables<SlotRow, MoveRow> t;
};

extern "C" void sicn_ragged_roi_move_free(sicn_ragged_roi_move *mv) { delete mv; }

extern "C" int sicn_ragged_roi_move_create(const sicn_ragged_coder *coder, const sicn_ragged_roi_slot *slots, int n_slots,
                                           sicn_ragged_roi_move **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    if (!coder || !slots || n_slots < 1) return SICN_EINVAL;
    sicn::RaggedCoderView v;
    sicn::ragged_coder_view(coder, &v);
    if (v.row_bytes != sizeof(CoderRow) || v.n_images < 1) return SICN_EINVAL;
    const CoderRow *rows = (const CoderRow *)v.rows_host;
    return sicn::make_object(out, [&](sicn_ragged_roi_move &mv) {
        const size_t n = (size_t)v.n_images;
        std::vector<uint32_t> lat_w(n), lat_h(n), wss(n), img_w(n), img_h(n);
        for (size_t i = 0; i < n; i++) {
            lat_w[i] = rows[i].lat_w; lat_h[i] = rows[i].lat_h; wss[i] = rows[i].wss; img_w[i] = rows[i].img_w; img_h[i] = rows[i].img_h;
        }
        std::vector<uint64_t> ws;
        std::vector<SlotRow> srows((size_t)n_slots);
        if (int rc = image_workspace_bytes(rows, v.n_images, v.ws_bytes, &ws)) return rc;
        if (int rc = sicn_roi_move::layout(lat_w.data(), lat_h.data(), rows[0].lat_c, wss.data(), img_w.data(), img_h.data(), ws.data(), v.n_images,
                                           slots, n_slots, srows.data(), nullptr, &mv.totals))
            return rc;
        sicn::ChipGeom chip;
        if (int rc = sicn::chip_geom(&chip)) return rc;       // no device, or not a gfx950 one
        mv.n_slots = n_slots;
        mv.d_rows = (const CoderRow *)v.d_rows;
        // the latency form (one 16 KB table) while all waves of the CAPACITY fit the chip at five per CU, the full decoder's rule
        mv.bigtab = mv.totals.items <= 5ull * (unsigned)chip.n_cu;
        sicn::ItemMap item_slot;
        for (size_t k = 0; k < srows.size(); k++) item_slot.add(srows[k].max_streams, (uint32_t)k);
        return item_slot.upload(mv.d_item_slot) && mv.t.build(srows) ? SICN_OK : SICN_ENOMEM;
    });
}

extern "C" size_t sicn_ragged_roi_move_workspace_bytes(const sicn_ragged_roi_move *mv) { return mv ? (size_t)mv->totals.workspace : 0; }

extern "C" int sicn_ragged_roi_move_decode_async(const sicn_ragged_roi_move *mv, const int32_t *xy_dev, const uint8_t *containers,
                                                 const sicn_codec_status *valid_dev_or_null, uint8_t *band, uint8_t *window_latent,
                                                 sicn_codec_status *status_dev, uint32_t *flags_dev, void *workspace, size_t workspace_bytes,
                                                 void *hip_stream)
{
    if (!mv || !xy_dev || !containers || !band || !window_latent || !status_dev || !flags_dev) return SICN_EINVAL;
    if (int rc = sicn::workspace_rc(workspace, workspace_bytes, mv->totals.workspace)) return rc;
    if (reinterpret_cast<uintptr_t>(xy_dev) & 3) return SICN_EINVAL;
    if (int rc = sicn::chip_geom(nullptr)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    const uint32_t *valid = (const uint32_t *)valid_dev_or_null;
    const unsigned n_slots = (unsigned)mv->n_slots, items = (unsigned)mv->totals.items;
    const auto &t = mv->t;
    hipLaunchKernelGGL(k_roi_place, dim3((n_slots + 63) / 64), dim3(64), 0, stream, xy_dev, t.d_srows.get(), n_slots, t.d_mrows.mut(),
                       t.d_lat_rows.mut(), t.d_pix_rows.mut(), flags_dev, t.d_origins.mut());
    if (mv->bigtab)
        hipLaunchKernelGGL(k_roi_move_decode<true>, dim3(items), dim3(64), 0, stream, containers, valid, band, ws, mv->d_rows, t.d_srows.get(),
                           t.d_mrows.get(), mv->d_item_slot.get());
    else
        hipLaunchKernelGGL(k_roi_move_decode<false>, dim3(items), dim3(64), 0, stream, containers, valid, band, ws, mv->d_rows, t.d_srows.get(),
                           t.d_mrows.get(), mv->d_item_slot.get());
    hipLaunchKernelGGL(k_roi_move_finish, dim3(n_slots), dim3(256), 0, stream, containers, valid, (uint32_t *)status_dev, ws, mv->d_rows,
                       t.d_srows.get(), t.d_mrows.get());
    if (hipGetLastError() != hipSuccess) return SICN_ENODEV;
    return t.cut(false, band, window_latent, hip_stream);
}

extern "C" const int32_t *sicn_ragged_roi_move_origins(const sicn_ragged_roi_move *mv) { return mv ? mv->t.d_origins.get() : nullptr; }

extern "C" int sicn_ragged_roi_move_cut_async(const sicn_ragged_roi_move *mv, const uint8_t *recon, uint8_t *roi_out, void *hip_stream)
{
    return mv ? mv->t.cut(true, recon, roi_out, hip_stream) : SICN_EINVAL;
}
