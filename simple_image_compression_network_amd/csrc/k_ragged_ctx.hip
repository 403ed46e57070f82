// Ragged context coder (include/sicn_ragged_ctx.h): the rANS-WC stages of k_ctx_body.hpp over n latents of n different shapes, six
// launches per encode and eight per decode for the whole batch.  The stages, CtxRow and ctx_image() are the uniform coder's
// (sicn_codec_ctx.inc); what differs is where a workgroup's row comes from: loaded from a table here, computed from blockIdx.y there.
// Behind them the window decoder (include/sicn_ragged_ctx_window.h): the decode stage over a SELECTION of every image's streams.
//
// Grids: flat over work items.
//   statistics          chunks of an image's dwords, ctx_hist_blocks(n_i) per image (the uniform coder's rule); one workgroup takes the
//                       byte statistics (stats_body) and the class histograms (ctx_hist_body) of its chunk
//   encode              groups of CTX_WPB streams, rounded up per image: a workgroup shares one copy of its image's class tables
//   decode              groups of CTX_WPB_DEC streams, rounded up per image AND per set: anchors of every image, then non-anchors
//   compaction          single streams
//   clear, tables, parse, scan + verdict, finish   one workgroup per image
// Two kinds of table, built on the host at creation:
//   chunk_image[], enc_image[], dec_image[2][], stream_image[] : the image a work item belongs to — ONE load resolves item -> image
//   rows[image]                                                : CtxRow, the image's geometry, its first work items and its 64-bit
//                                                                byte offsets in the latent / scale tensors, the slot buffer and the workspace
// Both loads are wave-uniform (they depend on blockIdx.x only) and stay in scalar registers.  Every kernel below: load the row of
// its image (load_row), resolve it (ctx_image), call the stage with the index inside the image.
#include <vector>

#include "../../include/sicn_ragged_ctx.h"
#include "../../include/sicn_ctx_stream_length.h"
#include "../../include/sicn_ragged_ctx_window.h"
#include "ctx_window_host.hpp"
#include "device_table.hpp"
#include "k_ctx_body.hpp"
#include "sicn_internal.h"

namespace {

// encoder, first on the stream: the statistics block and the class histograms of every image, which the next stage adds to
__global__ __launch_bounds__(256) void k_ragged_ctx_clear(uint8_t *__restrict__ workspace, const CtxRow *__restrict__ rows)
{
    ctx_clear_body(ctx_image(load_row(rows, blockIdx.x), nullptr, nullptr, nullptr, workspace));
}

// CLASSES: the encoder's statistics (byte histogram, checksum sums, class histograms); else the decoder's (checksum sums of what it decoded)
template <bool CLASSES>
__global__ __launch_bounds__(256) void k_ragged_ctx_stats(const uint8_t *__restrict__ latents, const uint8_t *__restrict__ scales,
                                                          uint8_t *__restrict__ workspace, const CtxRow *__restrict__ rows,
                                                          const uint32_t *__restrict__ chunk_image)
{
    const CtxRow r = load_row(rows, uni(chunk_image[blockIdx.x]));
    const CtxImage im = ctx_image(r, latents, scales, nullptr, workspace);
    const uint32_t local = blockIdx.x - r.first_chunk;
    stats_body(im.lat, r.g.W * r.g.H * r.g.C, im.w.hist, im.w.sums, nullptr, local, r.n_chunks);
    if constexpr (CLASSES) ctx_hist_body(im, local, r.n_chunks);
}

// valid: a sicn_codec_status array or nullptr
__global__ __launch_bounds__(64) void k_ragged_ctx_parse(const uint8_t *__restrict__ containers, const uint32_t *__restrict__ valid,
                                                         uint8_t *__restrict__ workspace, const CtxRow *__restrict__ rows)
{
    ctx_parse_body(ctx_image(load_row(rows, blockIdx.x), nullptr, nullptr, containers, workspace), valid, blockIdx.x);
}

// dec: the tables are read from the containers (and checked); else made from the class histograms and written to them, with the header
__global__ __launch_bounds__(1024) void k_ragged_ctx_tables(uint8_t *__restrict__ containers, uint8_t *__restrict__ workspace,
                                                            const CtxRow *__restrict__ rows, int dec)
{
    ctx_tables_body(ctx_image(load_row(rows, blockIdx.x), nullptr, nullptr, containers, workspace), dec);
}

__global__ __launch_bounds__(64 * CTX_WPB) void k_ragged_ctx_encode(const uint8_t *__restrict__ latents, const uint8_t *__restrict__ scales,
                                                                    uint8_t *__restrict__ workspace, const CtxRow *__restrict__ rows,
                                                                    const uint32_t *__restrict__ enc_image)
{
    const CtxRow r = load_row(rows, uni(enc_image[blockIdx.x]));
    ctx_encode_body(ctx_image(r, latents, scales, nullptr, workspace), blockIdx.x - r.first_enc);
}

// One workgroup per image: the scan stage, in the encoder behind the image's verdict on its statistics and tables (status.error)
__global__ __launch_bounds__(1024) void k_ragged_ctx_scan(uint8_t *__restrict__ containers, uint32_t *__restrict__ status,
                                                          uint8_t *__restrict__ workspace, const CtxRow *__restrict__ rows, int dec)
{
    const CtxImage im = ctx_image(load_row(rows, blockIdx.x), nullptr, nullptr, containers, workspace);
    if (dec) return ctx_scan_body(im, nullptr, blockIdx.x, true);
    if (threadIdx.x == 0) status[2 * (size_t)blockIdx.x] = ctx_enc_verdict(im.w.meta, im.w.hist);
    ctx_scan_body(im, status, blockIdx.x, false);
}

__global__ __launch_bounds__(256) void k_ragged_ctx_compact(uint8_t *__restrict__ containers, uint8_t *__restrict__ workspace,
                                                            const CtxRow *__restrict__ rows, const uint32_t *__restrict__ stream_image)
{
    const CtxRow r = load_row(rows, uni(stream_image[blockIdx.x]));
    ctx_compact_body(ctx_image(r, nullptr, nullptr, containers, workspace), blockIdx.x - r.first_stream);
}

// one set per launch (anchors first): dec_image is the table of that set
template <int SET>
__global__ __launch_bounds__(64 * CTX_WPB_DEC) void k_ragged_ctx_decode(const uint8_t *__restrict__ containers, const uint8_t *__restrict__ scales,
                                                                        uint8_t *__restrict__ latents, uint8_t *__restrict__ workspace,
                                                                        const CtxRow *__restrict__ rows, const uint32_t *__restrict__ dec_image)
{
    const CtxRow r = load_row(rows, uni(dec_image[blockIdx.x]));
    ctx_decode_body<SET>(ctx_image(r, latents, scales, containers, workspace), (blockIdx.x - r.first_dec[SET]) * CTX_WPB_DEC, r.g.nst[SET]);
}

// ---- the window decoder (include/sicn_ragged_ctx_window.h) ------------------------------------------------------------------------
// One set per launch, a flat grid over groups of CTX_WPB_DEC SELECTED streams of that set, rounded up per image.  Two wave-uniform
// loads resolve an item: win_image[item] -> image, then the coder's CtxRow and the window's CtxWinRow.  The decode stage runs with
// the stream's REAL index — offsets, geometry and the edge tests of the class rule are the image's own — on a latent pointer
// biased so that latent row band_row0 is the band's first: the symbols land in the band.  The scale map stays the image's full one.
struct CtxWinRow {
    uint64_t lat_bias;                  // band_offset - band_row0 * W * C, modulo 2^64: added to the band tensor's address
    uint32_t first[2], end[2];          // the selected streams per set, in the set's own numbering
    uint32_t first_item[2];             // the image's first work item in the flat grid of each set
    uint32_t symbols;                   // what the selected streams hold
    uint32_t pad;
};

template <int SET>
__global__ __launch_bounds__(64 * CTX_WPB_DEC) void k_ragged_ctx_decode_window(const uint8_t *__restrict__ containers,
                                                                               const uint8_t *__restrict__ scales, uint8_t *__restrict__ band,
                                                                               uint8_t *__restrict__ workspace, const CtxRow *__restrict__ rows,
                                                                               const CtxWinRow *__restrict__ wrows,
                                                                               const uint32_t *__restrict__ win_image)
{
    const uint32_t img = uni(win_image[blockIdx.x]);
    const CtxRow r = load_row(rows, img);
    const CtxWinRow *w = wrows + img;
    CtxImage im = ctx_image(r, nullptr, scales, containers, workspace);
    im.lat = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(band) + uni(w->lat_bias));
    ctx_decode_body<SET>(im, uni(w->first[SET]) + (blockIdx.x - uni(w->first_item[SET])) * CTX_WPB_DEC, uni(w->end[SET]));
}

// one workgroup per image: the verdict of the container's fixed part and of the selected streams; bit 7 is never set
__global__ __launch_bounds__(64) void k_ragged_ctx_finish_window(uint32_t *__restrict__ status, uint8_t *__restrict__ workspace,
                                                                 const CtxRow *__restrict__ rows, const CtxWinRow *__restrict__ wrows)
{
    if (threadIdx.x) return;
    ctx_finish_window_body(ctx_image(load_row(rows, blockIdx.x), nullptr, nullptr, nullptr, workspace), status, blockIdx.x,
                           wrows[blockIdx.x].symbols);
}

__global__ __launch_bounds__(64) void k_ragged_ctx_finish(uint32_t *__restrict__ status, uint8_t *__restrict__ workspace,
                                                          const CtxRow *__restrict__ rows)
{
    if (threadIdx.x) return;
    ctx_finish_body(ctx_image(load_row(rows, blockIdx.x), nullptr, nullptr, nullptr, workspace), status, blockIdx.x);
}

// ---- the layout: pure host --------------------------------------------------------------------------------------------------
struct Plan {
    std::vector<CtxRow> rows;
    uint64_t lat_bytes = 0, slot_bytes = 0, ws_bytes = 0, streams = 0, chunks = 0, enc_groups = 0, dec_groups[2] = {0, 0};
};

// keep_rows = false: totals only (nothing is allocated).  wss_or_null: the stream length of every image, NULL = 16384
int plan_ctx(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *wss_or_null, const uint32_t *img_w,
             const uint32_t *img_h, int n_images, bool keep_rows, sicn_ragged_ctx_image *images, Plan *p)
{
    if (!lat_w || !lat_h || n_images < 1) return SICN_EINVAL;
    if (keep_rows) p->rows.reserve((size_t)n_images);
    for (int i = 0; i < n_images; i++) {
        CtxRow r{};
        const uint32_t wss = wss_or_null ? wss_or_null[i] : WSS;
        if (int rc = ctx_row_shape(r, lat_w[i], lat_h[i], lat_c, img_w ? img_w[i] : 0, img_h ? img_h[i] : 0, wss)) return rc;
        const uint32_t n = r.g.W * r.g.H * r.g.C, ns = r.g.nst[0] + r.g.nst[1];
        const uint64_t slot = align_up(sicn_codec_ctx_max_bytes_sl(lat_w[i], lat_h[i], lat_c, wss), 16);   // (r.slot_cap is this, saturated)
        r.lat_off = p->lat_bytes;
        r.slot_off = p->slot_bytes;
        r.ws_off = p->ws_bytes;
        r.first_chunk = (uint32_t)p->chunks;
        r.first_enc = (uint32_t)p->enc_groups;
        r.first_dec[0] = (uint32_t)p->dec_groups[0];
        r.first_dec[1] = (uint32_t)p->dec_groups[1];
        r.first_stream = (uint32_t)p->streams;
        p->lat_bytes += n;
        p->slot_bytes += slot;
        p->ws_bytes += ctx_ws_bytes(ns, wss);
        p->streams += ns;
        p->chunks += r.n_chunks;
        p->enc_groups += (ns + CTX_WPB - 1) / CTX_WPB;
        for (int s = 0; s < 2; s++) p->dec_groups[s] += (r.g.nst[s] + CTX_WPB_DEC - 1) / CTX_WPB_DEC;
        if (p->streams >= (uint64_t)sicn::RAGGED_MAX_ITEMS || p->chunks >= (uint64_t)sicn::RAGGED_MAX_ITEMS) return SICN_EINVAL;
        if (images) images[i] = sicn_ragged_ctx_image{r.lat_off, r.slot_off, r.ws_off, slot, n, r.g.nst[0], r.g.nst[1]};
        if (keep_rows) p->rows.push_back(r);
    }
    return SICN_OK;
}

}  // namespace

struct sicn_ragged_ctx_coder {
    int n_images = 0;
    Plan plan;
    sicn::DeviceTable<CtxRow> d_rows;               // [n_images]
    sicn::DeviceTable<uint32_t> d_chunk_image;      // [chunks]
    sicn::DeviceTable<uint32_t> d_enc_image;        // [enc_groups]
    sicn::DeviceTable<uint32_t> d_dec_image[2];     // [dec_groups[set]]
    sicn::DeviceTable<uint32_t> d_stream_image;     // [streams]
};

extern "C" int sicn_ragged_ctx_layout_sl(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                                         int n_images, sicn_ragged_ctx_image *images_or_null, uint64_t totals[3])
{
    Plan p;
    if (int rc = plan_ctx(lat_w, lat_h, lat_c, stream_symbols_or_null, nullptr, nullptr, n_images, false, images_or_null, &p)) return rc;
    if (totals) {
        totals[0] = p.lat_bytes;
        totals[1] = p.slot_bytes;
        totals[2] = p.ws_bytes;
    }
    return SICN_OK;
}

extern "C" int sicn_ragged_ctx_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, int n_images,
                                      sicn_ragged_ctx_image *images_or_null, uint64_t totals[3])
{
    return sicn_ragged_ctx_layout_sl(lat_w, lat_h, lat_c, nullptr, n_images, images_or_null, totals);
}

extern "C" void sicn_ragged_ctx_coder_free(sicn_ragged_ctx_coder *coder) { delete coder; }

extern "C" int sicn_ragged_ctx_coder_create_sl(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c,
                                               const uint32_t *stream_symbols_or_null, const uint32_t *image_w_or_null,
                                               const uint32_t *image_h_or_null, int n_images, sicn_ragged_ctx_coder **out)
{
    return sicn::make_object(out, [&](sicn_ragged_ctx_coder &coder) {
        if (int rc = plan_ctx(lat_w, lat_h, lat_c, stream_symbols_or_null, image_w_or_null, image_h_or_null, n_images, true, nullptr, &coder.plan))
            return rc;
        if (int rc = sicn::chip_geom(nullptr)) return rc;       // no device, or not a gfx950 one
        coder.n_images = n_images;
        sicn::ItemMap chunk_image, enc_image, dec_image[2], stream_image;
        for (int i = 0; i < n_images; i++) {
            const CtxRow &r = coder.plan.rows[(size_t)i];
            const uint32_t ns = r.g.nst[0] + r.g.nst[1];
            chunk_image.add(r.n_chunks, (uint32_t)i);
            enc_image.add((ns + CTX_WPB - 1) / CTX_WPB, (uint32_t)i);
            for (int s = 0; s < 2; s++) dec_image[s].add((r.g.nst[s] + CTX_WPB_DEC - 1) / CTX_WPB_DEC, (uint32_t)i);
            stream_image.add(ns, (uint32_t)i);
        }
        const bool ok = coder.d_rows.upload(coder.plan.rows) && chunk_image.upload(coder.d_chunk_image) && enc_image.upload(coder.d_enc_image) &&
                        dec_image[0].upload(coder.d_dec_image[0]) && dec_image[1].upload(coder.d_dec_image[1]) &&
                        stream_image.upload(coder.d_stream_image);
        return ok ? SICN_OK : SICN_ENOMEM;
    });
}

extern "C" int sicn_ragged_ctx_coder_create(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *image_w_or_null,
                                            const uint32_t *image_h_or_null, int n_images, sicn_ragged_ctx_coder **out)
{
    return sicn_ragged_ctx_coder_create_sl(lat_w, lat_h, lat_c, nullptr, image_w_or_null, image_h_or_null, n_images, out);
}

void sicn::ragged_ctx_coder_view(const sicn_ragged_ctx_coder *coder, RaggedCoderView *v)
{
    v->n_images = coder->n_images;
    v->rows_host = coder->plan.rows.data();
    v->d_rows = coder->d_rows.get();
    v->row_bytes = sizeof(CtxRow);
    v->ws_bytes = coder->plan.ws_bytes;
}

extern "C" size_t sicn_ragged_ctx_coder_workspace_bytes(const sicn_ragged_ctx_coder *coder) { return coder ? (size_t)coder->plan.ws_bytes : 0; }

extern "C" int sicn_ragged_ctx_encode_async(const sicn_ragged_ctx_coder *coder, const uint8_t *latents, const uint8_t *scales,
                                            uint8_t *containers, sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes,
                                            void *hip_stream)
{
    if (!coder || !latents || !scales || !containers || !status_dev) return SICN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(latents) | reinterpret_cast<uintptr_t>(scales)) & 3) return SICN_EINVAL;   // dword gathers
    if (int rc = sicn::workspace_rc(workspace, workspace_bytes, coder->plan.ws_bytes)) return rc;
    if (int rc = sicn::chip_geom(nullptr)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    const Plan &p = coder->plan;
    const unsigned n = (unsigned)coder->n_images;
    // the uniform coder's stages (sicn_codec_ctx_encode_batch_async), its two statistics kernels as one and its verdict in the scan
    hipLaunchKernelGGL(k_ragged_ctx_clear, dim3(n), dim3(256), 0, stream, ws, coder->d_rows.get());
    hipLaunchKernelGGL(k_ragged_ctx_stats<true>, dim3((unsigned)p.chunks), dim3(256), 0, stream, latents, scales, ws, coder->d_rows.get(),
                       coder->d_chunk_image.get());
    hipLaunchKernelGGL(k_ragged_ctx_tables, dim3(n), dim3(1024), 0, stream, containers, ws, coder->d_rows.get(), 0);
    hipLaunchKernelGGL(k_ragged_ctx_encode, dim3((unsigned)p.enc_groups), dim3(64 * CTX_WPB), 0, stream, latents, scales, ws, coder->d_rows.get(),
                       coder->d_enc_image.get());
    hipLaunchKernelGGL(k_ragged_ctx_scan, dim3(n), dim3(1024), 0, stream, containers, (uint32_t *)status_dev, ws, coder->d_rows.get(), 0);
    hipLaunchKernelGGL(k_ragged_ctx_compact, dim3((unsigned)p.streams), dim3(256), 0, stream, containers, ws, coder->d_rows.get(),
                       coder->d_stream_image.get());
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_ragged_ctx_decode_async(const sicn_ragged_ctx_coder *coder, const uint8_t *containers,
                                            const sicn_codec_status *valid_dev_or_null, const uint8_t *scales, uint8_t *latents,
                                            sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!coder || !containers || !scales || !latents || !status_dev) return SICN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(latents) | reinterpret_cast<uintptr_t>(scales)) & 3) return SICN_EINVAL;
    if (reinterpret_cast<uintptr_t>(containers) & 1) return SICN_EINVAL;   // the streams are read as 16-bit words (slot offsets are even)
    if (int rc = sicn::workspace_rc(workspace, workspace_bytes, coder->plan.ws_bytes)) return rc;
    if (int rc = sicn::chip_geom(nullptr)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    uint8_t *slots = const_cast<uint8_t *>(containers);   // the tables and scan kernels write containers in the encoder only
    const Plan &p = coder->plan;
    const unsigned n = (unsigned)coder->n_images;
    // a non-anchor's class reads its neighbours' bytes whatever they hold: start from zeros so that a rejected container
    // cannot make the result depend on what the buffer held before.  First, so that a failure here leaves nothing enqueued.
    if (hipMemsetAsync(latents, 0, (size_t)p.lat_bytes, stream) != hipSuccess) return SICN_ENODEV;
    hipLaunchKernelGGL(k_ragged_ctx_parse, dim3(n), dim3(64), 0, stream, containers, (const uint32_t *)valid_dev_or_null, ws, coder->d_rows.get());
    hipLaunchKernelGGL(k_ragged_ctx_tables, dim3(n), dim3(1024), 0, stream, slots, ws, coder->d_rows.get(), 1);
    hipLaunchKernelGGL(k_ragged_ctx_scan, dim3(n), dim3(1024), 0, stream, slots, (uint32_t *)nullptr, ws, coder->d_rows.get(), 1);
    hipLaunchKernelGGL(k_ragged_ctx_decode<0>, dim3((unsigned)p.dec_groups[0]), dim3(64 * CTX_WPB_DEC), 0, stream, containers, scales, latents, ws,
                       coder->d_rows.get(), coder->d_dec_image[0].get());
    if (p.dec_groups[1])   // (a batch of 1 x 1 latents has no non-anchors)
        hipLaunchKernelGGL(k_ragged_ctx_decode<1>, dim3((unsigned)p.dec_groups[1]), dim3(64 * CTX_WPB_DEC), 0, stream, containers, scales, latents, ws,
                           coder->d_rows.get(), coder->d_dec_image[1].get());
    hipLaunchKernelGGL(k_ragged_ctx_stats<false>, dim3((unsigned)p.chunks), dim3(256), 0, stream, latents, scales, ws, coder->d_rows.get(),
                       coder->d_chunk_image.get());
    hipLaunchKernelGGL(k_ragged_ctx_finish, dim3(n), dim3(64), 0, stream, (uint32_t *)status_dev, ws, coder->d_rows.get());
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

// ---- the window decoder ----------------------------------------------------------------------------------------------------------
extern "C" int sicn_ragged_ctx_window_layout_sl(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c,
                                                const uint32_t *stream_symbols_or_null, const uint32_t *r0, const uint32_t *rh, int n_images,
                                                sicn_ragged_ctx_window_image *images_or_null, uint64_t totals[2])
{
    uint64_t coder[3] = {0, 0, 0}, band = 0;
    if (int rc = sicn_ragged_ctx_layout_sl(lat_w, lat_h, lat_c, stream_symbols_or_null, n_images, nullptr, coder)) return rc;
    if (int rc = sicn_ctx_window::window_layout_sl(lat_w, lat_h, lat_c, stream_symbols_or_null, r0, rh, n_images, images_or_null, &band, nullptr))
        return rc;
    if (totals) {
        totals[0] = band;
        totals[1] = coder[2];
    }
    return SICN_OK;
}

extern "C" int sicn_ragged_ctx_window_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *r0, const uint32_t *rh,
                                             int n_images, sicn_ragged_ctx_window_image *images_or_null, uint64_t totals[2])
{
    return sicn_ragged_ctx_window_layout_sl(lat_w, lat_h, lat_c, nullptr, r0, rh, n_images, images_or_null, totals);
}

struct sicn_ragged_ctx_window {
    int n_images = 0;
    uint64_t band_bytes = 0, ws_bytes = 0, groups[2] = {0, 0};
    const CtxRow *d_rows = nullptr;                  // the coder's
    sicn::DeviceTable<CtxWinRow> d_wrows;            // [n_images]
    sicn::DeviceTable<uint32_t> d_win_image[2];      // [groups[set]]
};

extern "C" void sicn_ragged_ctx_window_free(sicn_ragged_ctx_window *win) { delete win; }

extern "C" int sicn_ragged_ctx_window_create(const sicn_ragged_ctx_coder *coder, const uint32_t *r0, const uint32_t *rh,
                                             sicn_ragged_ctx_window **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    if (!coder || !r0 || !rh || coder->n_images < 1) return SICN_EINVAL;
    return sicn::make_object(out, [&](sicn_ragged_ctx_window &win) {
        const int n = coder->n_images;
        std::vector<CtxWinRow> wrows((size_t)n);
        sicn::ItemMap win_image[2];
        uint64_t at = 0;
        for (int i = 0; i < n; i++) {
            const CtxRow &r = coder->plan.rows[(size_t)i];
            sicn_ragged_ctx_window_image im;
            if (int rc = sicn_ctx_window::plan_of_sl(r.g.W, r.g.H, r.g.C, r.g.S, r0[i], rh[i], at, &im)) return rc;
            CtxWinRow w{};
            w.lat_bias = at - (uint64_t)im.band_row0 * r.g.W * r.g.C;
            w.symbols = im.symbols;
            for (int s = 0; s < 2; s++) {
                w.first[s] = im.first_stream[s];
                w.end[s] = im.end_stream[s];
                // <= the coder's groups, which fit a grid
                w.first_item[s] = win_image[s].add((im.end_stream[s] - im.first_stream[s] + CTX_WPB_DEC - 1) / CTX_WPB_DEC, (uint32_t)i);
            }
            wrows[(size_t)i] = w;
            at += sicn_ctx_window::a16(im.band_bytes);
        }
        if (int rc = sicn::chip_geom(nullptr)) return rc;       // no device, or not a gfx950 one
        win.n_images = n;
        win.band_bytes = at;
        win.ws_bytes = coder->plan.ws_bytes;
        win.d_rows = coder->d_rows.get();
        for (int s = 0; s < 2; s++) win.groups[s] = win_image[s].size();
        const bool ok = win.d_wrows.upload(wrows) && win_image[0].upload(win.d_win_image[0]) && win_image[1].upload(win.d_win_image[1]);
        return ok ? SICN_OK : SICN_ENOMEM;
    });
}

extern "C" size_t sicn_ragged_ctx_window_workspace_bytes(const sicn_ragged_ctx_window *win) { return win ? (size_t)win->ws_bytes : 0; }

extern "C" int sicn_ragged_ctx_window_decode_async(const sicn_ragged_ctx_window *win, const uint8_t *containers,
                                                   const sicn_codec_status *valid_dev_or_null, const uint8_t *scales, uint8_t *band,
                                                   sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!win || !containers || !scales || !band || !status_dev) return SICN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(band) | reinterpret_cast<uintptr_t>(scales)) & 3) return SICN_EINVAL;   // dword gathers
    if (reinterpret_cast<uintptr_t>(containers) & 1) return SICN_EINVAL;   // the streams are read as 16-bit words (slot offsets are even)
    if (int rc = sicn::workspace_rc(workspace, workspace_bytes, win->ws_bytes)) return rc;
    if (int rc = sicn::chip_geom(nullptr)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    uint8_t *slots = const_cast<uint8_t *>(containers);   // the tables and scan kernels write containers in the encoder only
    const unsigned n = (unsigned)win->n_images;
    // the full decoder's reason: a non-anchor's class reads its neighbours' bytes whatever they hold.  First, so that a failure here
    // leaves nothing enqueued.
    if (hipMemsetAsync(band, 0, (size_t)win->band_bytes, stream) != hipSuccess) return SICN_ENODEV;
    hipLaunchKernelGGL(k_ragged_ctx_parse, dim3(n), dim3(64), 0, stream, containers, (const uint32_t *)valid_dev_or_null, ws, win->d_rows);
    hipLaunchKernelGGL(k_ragged_ctx_tables, dim3(n), dim3(1024), 0, stream, slots, ws, win->d_rows, 1);
    hipLaunchKernelGGL(k_ragged_ctx_scan, dim3(n), dim3(1024), 0, stream, slots, (uint32_t *)nullptr, ws, win->d_rows, 1);
    hipLaunchKernelGGL(k_ragged_ctx_decode_window<0>, dim3((unsigned)win->groups[0]), dim3(64 * CTX_WPB_DEC), 0, stream, containers, scales, band,
                       ws, win->d_rows, win->d_wrows.get(), win->d_win_image[0].get());
    if (win->groups[1])   // (a window of rows without non-anchors, e.g. of 1 x 1 latents)
        hipLaunchKernelGGL(k_ragged_ctx_decode_window<1>, dim3((unsigned)win->groups[1]), dim3(64 * CTX_WPB_DEC), 0, stream, containers, scales,
                           band, ws, win->d_rows, win->d_wrows.get(), win->d_win_image[1].get());
    hipLaunchKernelGGL(k_ragged_ctx_finish_window, dim3(n), dim3(64), 0, stream, (uint32_t *)status_dev, ws, win->d_rows, win->d_wrows.get());
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}
