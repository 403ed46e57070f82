// Moving ROI decode of the hyperprior configuration (include/sicn_ragged_ctx_roi_move.h): the rANS-WC window decoder of
// k_ragged_ctx.hip over SLOTS whose rectangles are placed on the device, from positions read out of device memory on every call,
// split into what a set of containers fixes (prepare: parse, tables, scan) and what a move fixes (decode).  A translation unit of its
// own: the kernels of k_ragged_ctx.hip, k_ragged_roi_move.hip, k_ragged_window.hip and sicn_codec.hip keep their code as it is; the
// stages are k_ctx_body.hpp's, called unchanged.  The two cuts are k_ragged_window.hip's k_ragged_cut itself
// (sicn::ragged_cut_launch) over rows this file writes.
//
// Tables.  What no coder changes is k_roi_move_common.hpp's MoveTables, shared with k_ragged_roi_move.hip: srows[slot] (SlotRow of
// ctx_roi_move_host.hpp: the shared SlotGeom, then the slot's meta block, its first decode items and max_streams per set, the band's
// row capacity and its image's stream length), the two cuts' item -> slot maps, and the rows k_ctx_roi_place writes on the stream,
// one thread per slot, from place_slot() — the function the host entry points call too: mrows[slot] (MoveRow, the streams
// [first, end) of each set the slot selects now and where they land in its band), lat_rows[slot], pix_rows[slot], and the caller's
// flags[slot].  This file's own:
//   item_slot[set][]   : the slot of a work item of a set's decode grid (sum of ceil(max_streams[set] / CTX_WPB_DEC)) — ONE load
//                        resolves item -> slot
//   images[]           : the DISTINCT images the slots name, ascending: the grid of the three prepare kernels
//   rows[image]        : the CODER's CtxRow table
//   the slot's meta block of the workspace <- its image's meta[0..3] as prepare left them, written by k_ctx_roi_place: what this
//   call's streams report lands there and nowhere else, and what the last call's reported is gone
// Every kernel below has the shape of k_ragged_ctx.hip's: load the row of its image (load_row), resolve it (ctx_image), call the stage.
#include <vector>

#include "../../include/sicn_ragged_ctx_roi_move.h"
#include "../../include/sicn_ctx_stream_length.h"
#include "ctx_roi_move_host.hpp"
#include "k_ctx_body.hpp"
#include "../../include/sicn_ragged_rect.h"
#include "k_roi_move_common.hpp"

namespace {

using sicn_ctx_roi_move::MoveRow;
using sicn_ctx_roi_move::SlotRow;
using sicn_window::CutRow;

static_assert(sicn_ctx_roi_move::WPB_DEC == CTX_WPB_DEC, "the layout's streams per work item are the decode stage's");
static_assert(sicn_ctx_roi_move::META_BYTES == 64, "a slot's block is one meta block of ctx_carve");

// ---- prepare: the container's fixed part of the DISTINCT images the slots name, once per set of containers -----------------------
__global__ __launch_bounds__(64) void k_ctx_roi_parse(const uint8_t *__restrict__ containers, const uint32_t *__restrict__ valid,
                                                      uint8_t *__restrict__ workspace, const CtxRow *__restrict__ rows,
                                                      const uint32_t *__restrict__ images)
{
    const uint32_t img = uni(images[blockIdx.x]);
    ctx_parse_body(ctx_image(load_row(rows, img), nullptr, nullptr, containers, workspace), valid, img);
}

__global__ __launch_bounds__(1024) void k_ctx_roi_tables(const uint8_t *__restrict__ containers, uint8_t *__restrict__ workspace,
                                                         const CtxRow *__restrict__ rows, const uint32_t *__restrict__ images)
{
    ctx_tables_body(ctx_image(load_row(rows, uni(images[blockIdx.x])), nullptr, nullptr, containers, workspace), true);
}

__global__ __launch_bounds__(1024) void k_ctx_roi_scan(const uint8_t *__restrict__ containers, uint8_t *__restrict__ workspace,
                                                       const CtxRow *__restrict__ rows, const uint32_t *__restrict__ images)
{
    const uint32_t img = uni(images[blockIdx.x]);
    ctx_scan_body(ctx_image(load_row(rows, img), nullptr, nullptr, containers, workspace), nullptr, img, true);
}

// ---- decode: once per move --------------------------------------------------------------------------------------------------------
// One thread per slot; nothing here is wave-uniform, so the image's row is read in place (load_row is for uniform rows).
__global__ __launch_bounds__(64) void k_ctx_roi_place(const int32_t *__restrict__ xy, const SlotRow *__restrict__ srows, uint32_t n_slots,
                                                      const CtxRow *__restrict__ rows, uint8_t *__restrict__ workspace,
                                                      MoveRow *__restrict__ mrows, CutRow *__restrict__ lat_rows, CutRow *__restrict__ pix_rows,
                                                      uint32_t *__restrict__ flags, int32_t *__restrict__ origins)
{
    const uint32_t slot = blockIdx.x * 64u + threadIdx.x;
    if (slot >= n_slots) return;
    const SlotRow s = srows[slot];
    sicn_roi_move::store_placement(slot, sicn_ctx_roi_move::place_slot(s, xy[2 * (size_t)slot], xy[2 * (size_t)slot + 1]), mrows, lat_rows,
                                   pix_rows, flags, origins);
    const CtxRow *r = rows + s.image;
    CtxWorkspace w;
    ctx_carve(w, workspace + r->ws_off, r->g.nst[0] + r->g.nst[1], wstream_cap(r->g.S));
    uint32_t *meta = reinterpret_cast<uint32_t *>(workspace + s.meta_off);
#pragma unroll
    for (int i = 0; i < 16; i++) meta[i] = i < 4 ? w.meta[i] : 0u;
}

// the slot's image as the stages see it: the coder's row, with the error words the slot's own
__device__ __forceinline__ CtxImage slot_image(const CtxRow *__restrict__ rows, const SlotRow *__restrict__ s, const uint8_t *scales,
                                               const uint8_t *containers, uint8_t *workspace)
{
    CtxImage im = ctx_image(load_row(rows, uni(s->image)), nullptr, scales, containers, workspace);
    im.w.meta = reinterpret_cast<uint32_t *>(workspace + uni((uint64_t)s->meta_off));
    return im;
}

// One set per launch, a flat grid FIXED by the capacities: groups of CTX_WPB_DEC streams, rounded up per slot.  A surplus item (its
// first stream >= end[SET] at this position) returns before it reads anything else or loads a table.
template <int SET>
__global__ __launch_bounds__(64 * CTX_WPB_DEC) void k_ctx_roi_move_decode(const uint8_t *__restrict__ containers, const uint8_t *__restrict__ scales,
                                                                          uint8_t *__restrict__ band, uint8_t *__restrict__ workspace,
                                                                          const CtxRow *__restrict__ rows, const SlotRow *__restrict__ srows,
                                                                          const MoveRow *__restrict__ mrows,
                                                                          const uint32_t *__restrict__ item_slot)
{
    const uint32_t slot = uni(item_slot[blockIdx.x]);
    const SlotRow *s = srows + slot;
    const MoveRow *m = mrows + slot;
    const uint32_t first = uni(m->first[SET]) + (blockIdx.x - uni(s->first_item[SET])) * CTX_WPB_DEC, end = uni(m->end[SET]);
    if (first >= end) return;                                // the capacity's surplus over this position's selection
    CtxImage im = slot_image(rows, s, scales, containers, workspace);
    im.lat = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(band) + uni((uint64_t)m->lat_bias));
    ctx_decode_body<SET>(im, first, end);
}

// one workgroup per slot: the verdict of the container's fixed part and of the streams the slot selected in this call
__global__ __launch_bounds__(64) void k_ctx_roi_move_finish(uint32_t *__restrict__ status, uint8_t *__restrict__ workspace,
                                                            const CtxRow *__restrict__ rows, const SlotRow *__restrict__ srows,
                                                            const MoveRow *__restrict__ mrows)
{
    if (threadIdx.x) return;
    const uint32_t slot = blockIdx.x;
    ctx_finish_window_body(slot_image(rows, srows + slot, nullptr, nullptr, workspace), status, slot, mrows[slot].symbols);   // one pair per SLOT
}

}  // namespace

// ---- capacity, placement, layout: pure host ------------------------------------------------------------------------------------
extern "C" int sicn_ragged_ctx_roi_move_capacity(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t stream_symbols, uint32_t rh_cap,
                                                 uint32_t cap[3])
{
    return sicn_ctx_roi_move::capacity(lat_w, lat_h, lat_c, stream_symbols, rh_cap, cap);
}

extern "C" int sicn_ragged_ctx_roi_move_place(int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, uint32_t lat_c,
                                              uint32_t stream_symbols, int32_t w, int32_t h, int32_t x0, int32_t y0, uint64_t band_offset,
                                              sicn_ragged_ctx_roi_placed *out)
{
    return sicn_ctx_roi_move::place(image_w, image_h, lat_w, lat_h, lat_c, stream_symbols, w, h, x0, y0, band_offset, out);
}

extern "C" int sicn_ragged_ctx_roi_move_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                                               const uint32_t *image_w, const uint32_t *image_h, int n_images, const sicn_ragged_roi_slot *slots,
                                               int n_slots, sicn_ragged_ctx_roi_move_slot *slots_out_or_null, uint64_t totals[7])
{
    if (!image_w || !image_h || !slots || n_slots < 1 || n_images < 1) return SICN_EINVAL;
    uint64_t coder[3] = {0, 0, 0};
    if (int rc = sicn_ragged_ctx_layout_sl(lat_w, lat_h, lat_c, stream_symbols_or_null, n_images, nullptr, coder)) return rc;
    sicn_ctx_roi_move::Totals t;
    if (int rc = sicn_ctx_roi_move::layout(lat_w, lat_h, lat_c, stream_symbols_or_null, image_w, image_h, coder[2], n_images, slots, n_slots,
                                           nullptr, slots_out_or_null, &t))
        return rc;
    if (totals) {
        totals[0] = t.band; totals[1] = t.latent; totals[2] = t.recon; totals[3] = t.roi; totals[4] = t.workspace;
        totals[5] = t.items[0]; totals[6] = t.items[1];
    }
    return SICN_OK;
}

// ---- the object ------------------------------------------------------------------------------------------------------------------
struct sicn_ragged_ctx_roi_move {
    int n_slots = 0, n_distinct = 0;
    sicn_ctx_roi_move::Totals totals;
    const CtxRow *d_rows = nullptr;         // the coder's
    sicn::DeviceTable<uint32_t> d_item_slot[2], d_images;
    sicn_roi_move::MoveTables<SlotRow, MoveRow> t;
};

extern "C" void sicn_ragged_ctx_roi_move_free(sicn_ragged_ctx_roi_move *mv) { delete mv; }

extern "C" int sicn_ragged_ctx_roi_move_create(const sicn_ragged_ctx_coder *coder, const sicn_ragged_roi_slot *slots, int n_slots,
                                               sicn_ragged_ctx_roi_move **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    if (!coder || !slots || n_slots < 1) return SICN_EINVAL;
    sicn::RaggedCoderView v;
    sicn::ragged_ctx_coder_view(coder, &v);
    if (v.row_bytes != sizeof(CtxRow) || v.n_images < 1) return SICN_EINVAL;
    const CtxRow *rows = (const CtxRow *)v.rows_host;
    return sicn::make_object(out, [&](sicn_ragged_ctx_roi_move &mv) {
        const size_t n = (size_t)v.n_images;
        std::vector<uint32_t> lat_w(n), lat_h(n), wss(n), img_w(n), img_h(n);
        for (size_t i = 0; i < n; i++) {
            lat_w[i] = rows[i].g.W; lat_h[i] = rows[i].g.H; wss[i] = rows[i].g.S; img_w[i] = rows[i].img_w; img_h[i] = rows[i].img_h;
        }
        std::vector<SlotRow> srows((size_t)n_slots);
        if (int rc = sicn_ctx_roi_move::layout(lat_w.data(), lat_h.data(), rows[0].g.C, wss.data(), img_w.data(), img_h.data(), v.ws_bytes,
                                               v.n_images, slots, n_slots, srows.data(), nullptr, &mv.totals))
            return rc;
        if (int rc = sicn::chip_geom(nullptr)) return rc;       // no device, or not a gfx950 one
        mv.n_slots = n_slots;
        mv.d_rows = (const CtxRow *)v.d_rows;
        sicn::ItemMap item_slot[2];
        std::vector<uint32_t> images;
        std::vector<char> named(n, 0);
        for (size_t k = 0; k < srows.size(); k++) {
            const SlotRow &s = srows[k];
            for (int set = 0; set < 2; set++) item_slot[set].add((s.max_streams[set] + CTX_WPB_DEC - 1) / CTX_WPB_DEC, (uint32_t)k);
            named[s.image] = 1;
        }
        for (size_t i = 0; i < n; i++)
            if (named[i]) images.push_back((uint32_t)i);
        mv.n_distinct = (int)images.size();
        const bool ok = item_slot[0].upload(mv.d_item_slot[0]) && item_slot[1].upload(mv.d_item_slot[1]) && mv.d_images.upload(images) &&
                        mv.t.build(srows);
        return ok ? SICN_OK : SICN_ENOMEM;
    });
}

extern "C" size_t sicn_ragged_ctx_roi_move_workspace_bytes(const sicn_ragged_ctx_roi_move *mv) { return mv ? (size_t)mv->totals.workspace : 0; }

extern "C" int sicn_ragged_ctx_roi_move_prepare_async(const sicn_ragged_ctx_roi_move *mv, const uint8_t *containers,
                                                      const sicn_codec_status *valid_dev_or_null, void *workspace, size_t workspace_bytes,
                                                      void *hip_stream)
{
    if (!mv || !containers) return SICN_EINVAL;
    if (reinterpret_cast<uintptr_t>(containers) & 1) return SICN_EINVAL;   // the streams are read as 16-bit words (slot offsets are even)
    if (int rc = sicn::workspace_rc(workspace, workspace_bytes, mv->totals.workspace)) return rc;
    if (int rc = sicn::chip_geom(nullptr)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    const unsigned n = (unsigned)mv->n_distinct;
    hipLaunchKernelGGL(k_ctx_roi_parse, dim3(n), dim3(64), 0, stream, containers, (const uint32_t *)valid_dev_or_null, ws, mv->d_rows,
                       mv->d_images.get());
    hipLaunchKernelGGL(k_ctx_roi_tables, dim3(n), dim3(1024), 0, stream, containers, ws, mv->d_rows, mv->d_images.get());
    hipLaunchKernelGGL(k_ctx_roi_scan, dim3(n), dim3(1024), 0, stream, containers, ws, mv->d_rows, mv->d_images.get());
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_ragged_ctx_roi_move_decode_async(const sicn_ragged_ctx_roi_move *mv, const int32_t *xy_dev, const uint8_t *containers,
                                                     const uint8_t *scales, uint8_t *band, uint8_t *window_latent,
                                                     sicn_codec_status *status_dev, uint32_t *flags_dev, void *workspace, size_t workspace_bytes,
                                                     void *hip_stream)
{
    if (!mv || !xy_dev || !containers || !scales || !band || !window_latent || !status_dev || !flags_dev) return SICN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(band) | reinterpret_cast<uintptr_t>(scales)) & 3) return SICN_EINVAL;   // dword gathers
    if (reinterpret_cast<uintptr_t>(containers) & 1) return SICN_EINVAL;
    if (int rc = sicn::workspace_rc(workspace, workspace_bytes, mv->totals.workspace)) return rc;
    if (reinterpret_cast<uintptr_t>(xy_dev) & 3) return SICN_EINVAL;
    if (int rc = sicn::chip_geom(nullptr)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    const unsigned n_slots = (unsigned)mv->n_slots;
    const auto &t = mv->t;
    hipLaunchKernelGGL(k_ctx_roi_place, dim3((n_slots + 63) / 64), dim3(64), 0, stream, xy_dev, t.d_srows.get(), n_slots, mv->d_rows, ws,
                       t.d_mrows.mut(), t.d_lat_rows.mut(), t.d_pix_rows.mut(), flags_dev, t.d_origins.mut());
    // the full decoder's reason: a non-anchor's class reads its neighbours' bytes whatever they hold
    if (hipMemsetAsync(band, 0, (size_t)mv->totals.band, stream) != hipSuccess) return SICN_ENODEV;
    hipLaunchKernelGGL(k_ctx_roi_move_decode<0>, dim3((unsigned)mv->totals.items[0]), dim3(64 * CTX_WPB_DEC), 0, stream, containers, scales, band, ws,
                       mv->d_rows, t.d_srows.get(), t.d_mrows.get(), mv->d_item_slot[0].get());
    if (mv->totals.items[1])   // (slots on 1 x 1 latents have no non-anchor capacity)
        hipLaunchKernelGGL(k_ctx_roi_move_decode<1>, dim3((unsigned)mv->totals.items[1]), dim3(64 * CTX_WPB_DEC), 0, stream, containers, scales, band,
                           ws, mv->d_rows, t.d_srows.get(), t.d_mrows.get(), mv->d_item_slot[1].get());
    hipLaunchKernelGGL(k_ctx_roi_move_finish, dim3(n_slots), dim3(64), 0, stream, (uint32_t *)status_dev, ws, mv->d_rows, t.d_srows.get(),
                       t.d_mrows.get());
    if (hipGetLastError() != hipSuccess) return SICN_ENODEV;
    return t.cut(false, band, window_latent, hip_stream);
}

extern "C" const int32_t *sicn_ragged_ctx_roi_move_origins(const sicn_ragged_ctx_roi_move *mv)
{
    return mv ? mv->t.d_origins.get() : nullptr;
}

extern "C" int sicn_ragged_ctx_roi_move_cut_async(const sicn_ragged_ctx_roi_move *mv, const uint8_t *recon, uint8_t *roi_out, void *hip_stream)
{
    return mv ? mv->t.cut(true, recon, roi_out, hip_stream) : SICN_EINVAL;
}
