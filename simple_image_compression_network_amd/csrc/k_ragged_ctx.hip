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
#include <new>
#include <vector>

#include "../../include/sicn_ragged_ctx.h"
#include "../../include/sicn_ctx_stream_length.h"
#include "../../include/sicn_ragged_ctx_window.h"
#include "ctx_window_host.hpp"
#include "k_ctx_body.hpp"
#include "sicn_internal.h"
#include "sicn_weights_io.h"

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
    CtxRow *d_rows = nullptr;                 // [n_images]
    uint32_t *d_chunk_image = nullptr;        // [chunks]
    uint32_t *d_enc_image = nullptr;          // [enc_groups]
    uint32_t *d_dec_image[2] = {nullptr, nullptr};   // [dec_groups[set]]
    uint32_t *d_stream_image = nullptr;       // [streams]
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

extern "C" void sicn_ragged_ctx_coder_free(sicn_ragged_ctx_coder *coder)
{
    if (!coder) return;
    for (void *p : {(void *)coder->d_rows, (void *)coder->d_chunk_image, (void *)coder->d_enc_image, (void *)coder->d_dec_image[0],
                    (void *)coder->d_dec_image[1], (void *)coder->d_stream_image})
        if (p) (void)hipFree(p);
    delete coder;
}

extern "C" int sicn_ragged_ctx_coder_create_sl(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c,
                                               const uint32_t *stream_symbols_or_null, const uint32_t *image_w_or_null,
                                               const uint32_t *image_h_or_null, int n_images, sicn_ragged_ctx_coder **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    sicn_ragged_ctx_coder *coder = new (std::nothrow) sicn_ragged_ctx_coder();
    if (!coder) return SICN_ENOMEM;
    int rc = SICN_OK;
    try {
        rc = plan_ctx(lat_w, lat_h, lat_c, stream_symbols_or_null, image_w_or_null, image_h_or_null, n_images, true, nullptr, &coder->plan);
        if (!rc) rc = sicn::chip_geom(nullptr);       // no device, or not a gfx950 one
        if (!rc) {
            coder->n_images = n_images;
            const Plan &p = coder->plan;
            std::vector<uint32_t> chunk_image, enc_image, dec_image[2], stream_image;
            chunk_image.reserve((size_t)p.chunks);
            enc_image.reserve((size_t)p.enc_groups);
            stream_image.reserve((size_t)p.streams);
            for (int i = 0; i < n_images; i++) {
                const CtxRow &r = p.rows[(size_t)i];
                const uint32_t ns = r.g.nst[0] + r.g.nst[1];
                chunk_image.insert(chunk_image.end(), (size_t)r.n_chunks, (uint32_t)i);
                enc_image.insert(enc_image.end(), (size_t)((ns + CTX_WPB - 1) / CTX_WPB), (uint32_t)i);
                for (int s = 0; s < 2; s++)
                    dec_image[s].insert(dec_image[s].end(), (size_t)((r.g.nst[s] + CTX_WPB_DEC - 1) / CTX_WPB_DEC), (uint32_t)i);
                stream_image.insert(stream_image.end(), (size_t)ns, (uint32_t)i);
            }
            auto up = [](const std::vector<uint32_t> &v, uint32_t **dev) { return v.empty() || sicn::upload(v.data(), v.size() * sizeof(uint32_t), dev); };
            if (!sicn::upload(p.rows.data(), p.rows.size() * sizeof(CtxRow), &coder->d_rows) || !up(chunk_image, &coder->d_chunk_image) ||
                !up(enc_image, &coder->d_enc_image) || !up(dec_image[0], &coder->d_dec_image[0]) ||
                !up(dec_image[1], &coder->d_dec_image[1]) || !up(stream_image, &coder->d_stream_image))
                rc = SICN_ENOMEM;
        }
    } catch (const std::bad_alloc &) { rc = SICN_ENOMEM; }
    if (rc) {
        sicn_ragged_ctx_coder_free(coder);
        return rc;
    }
    *out = coder;
    return SICN_OK;
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
    v->d_rows = coder->d_rows;
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
    if (!workspace || workspace_bytes < coder->plan.ws_bytes) return SICN_ENOSPC;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return SICN_EINVAL;
    if (int rc = sicn::chip_geom(nullptr)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    const Plan &p = coder->plan;
    const unsigned n = (unsigned)coder->n_images;
    // the uniform coder's stages (sicn_codec_ctx_encode_batch_async), its two statistics kernels as one and its verdict in the scan
    hipLaunchKernelGGL(k_ragged_ctx_clear, dim3(n), dim3(256), 0, stream, ws, coder->d_rows);
    hipLaunchKernelGGL(k_ragged_ctx_stats<true>, dim3((unsigned)p.chunks), dim3(256), 0, stream, latents, scales, ws, coder->d_rows,
                       coder->d_chunk_image);
    hipLaunchKernelGGL(k_ragged_ctx_tables, dim3(n), dim3(1024), 0, stream, containers, ws, coder->d_rows, 0);
    hipLaunchKernelGGL(k_ragged_ctx_encode, dim3((unsigned)p.enc_groups), dim3(64 * CTX_WPB), 0, stream, latents, scales, ws, coder->d_rows,
                       coder->d_enc_image);
    hipLaunchKernelGGL(k_ragged_ctx_scan, dim3(n), dim3(1024), 0, stream, containers, (uint32_t *)status_dev, ws, coder->d_rows, 0);
    hipLaunchKernelGGL(k_ragged_ctx_compact, dim3((unsigned)p.streams), dim3(256), 0, stream, containers, ws, coder->d_rows,
                       coder->d_stream_image);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_ragged_ctx_decode_async(const sicn_ragged_ctx_coder *coder, const uint8_t *containers,
                                            const sicn_codec_status *valid_dev_or_null, const uint8_t *scales, uint8_t *latents,
                                            sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!coder || !containers || !scales || !latents || !status_dev) return SICN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(latents) | reinterpret_cast<uintptr_t>(scales)) & 3) return SICN_EINVAL;
    if (reinterpret_cast<uintptr_t>(containers) & 1) return SICN_EINVAL;   // the streams are read as 16-bit words (slot offsets are even)
    if (!workspace || workspace_bytes < coder->plan.ws_bytes) return SICN_ENOSPC;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return SICN_EINVAL;
    if (int rc = sicn::chip_geom(nullptr)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    uint8_t *slots = const_cast<uint8_t *>(containers);   // the tables and scan kernels write containers in the encoder only
    const Plan &p = coder->plan;
    const unsigned n = (unsigned)coder->n_images;
    // a non-anchor's class reads its neighbours' bytes whatever they hold: start from zeros so that a rejected container
    // cannot make the result depend on what the buffer held before.  First, so that a failure here leaves nothing enqueued.
    if (hipMemsetAsync(latents, 0, (size_t)p.lat_bytes, stream) != hipSuccess) return SICN_ENODEV;
    hipLaunchKernelGGL(k_ragged_ctx_parse, dim3(n), dim3(64), 0, stream, containers, (const uint32_t *)valid_dev_or_null, ws, coder->d_rows);
    hipLaunchKernelGGL(k_ragged_ctx_tables, dim3(n), dim3(1024), 0, stream, slots, ws, coder->d_rows, 1);
    hipLaunchKernelGGL(k_ragged_ctx_scan, dim3(n), dim3(1024), 0, stream, slots, (uint32_t *)nullptr, ws, coder->d_rows, 1);
    hipLaunchKernelGGL(k_ragged_ctx_decode<0>, dim3((unsigned)p.dec_groups[0]), dim3(64 * CTX_WPB_DEC), 0, stream, containers, scales, latents, ws,
                       coder->d_rows, coder->d_dec_image[0]);
    if (p.dec_groups[1])   // (a batch of 1 x 1 latents has no non-anchors)
        hipLaunchKernelGGL(k_ragged_ctx_decode<1>, dim3((unsigned)p.dec_groups[1]), dim3(64 * CTX_WPB_DEC), 0, stream, containers, scales, latents, ws,
                           coder->d_rows, coder->d_dec_image[1]);
    hipLaunchKernelGGL(k_ragged_ctx_stats<false>, dim3((unsigned)p.chunks), dim3(256), 0, stream, latents, scales, ws, coder->d_rows,
                       coder->d_chunk_image);
    hipLaunchKernelGGL(k_ragged_ctx_finish, dim3(n), dim3(64), 0, stream, (uint32_t *)status_dev, ws, coder->d_rows);
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
    CtxWinRow *d_wrows = nullptr;                    // [n_images]
    uint32_t *d_win_image[2] = {nullptr, nullptr};   // [groups[set]]
};

extern "C" void sicn_ragged_ctx_window_free(sicn_ragged_ctx_window *win)
{
    if (!win) return;
    for (void *p : {(void *)win->d_wrows, (void *)win->d_win_image[0], (void *)win->d_win_image[1]})
        if (p) (void)hipFree(p);
    delete win;
}

extern "C" int sicn_ragged_ctx_window_create(const sicn_ragged_ctx_coder *coder, const uint32_t *r0, const uint32_t *rh,
                                             sicn_ragged_ctx_window **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    if (!coder || !r0 || !rh || coder->n_images < 1) return SICN_EINVAL;
    sicn_ragged_ctx_window *win = new (std::nothrow) sicn_ragged_ctx_window();
    if (!win) return SICN_ENOMEM;
    int rc = SICN_OK;
    try {
        const int n = coder->n_images;
        std::vector<CtxWinRow> wrows((size_t)n);
        std::vector<uint32_t> win_image[2];
        uint64_t at = 0;
        for (int i = 0; !rc && i < n; i++) {
            const CtxRow &r = coder->plan.rows[(size_t)i];
            sicn_ragged_ctx_window_image im;
            rc = sicn_ctx_window::plan_of_sl(r.g.W, r.g.H, r.g.C, r.g.S, r0[i], rh[i], at, &im);
            if (rc) break;
            CtxWinRow w{};
            w.lat_bias = at - (uint64_t)im.band_row0 * r.g.W * r.g.C;
            w.symbols = im.symbols;
            for (int s = 0; s < 2; s++) {
                w.first[s] = im.first_stream[s];
                w.end[s] = im.end_stream[s];
                w.first_item[s] = (uint32_t)win_image[s].size();       // <= the coder's groups, which fit a grid
                win_image[s].insert(win_image[s].end(), (size_t)((im.end_stream[s] - im.first_stream[s] + CTX_WPB_DEC - 1) / CTX_WPB_DEC), (uint32_t)i);
            }
            wrows[(size_t)i] = w;
            at += sicn_ctx_window::a16(im.band_bytes);
        }
        if (!rc) rc = sicn::chip_geom(nullptr);       // no device, or not a gfx950 one
        if (!rc) {
            win->n_images = n;
            win->band_bytes = at;
            win->ws_bytes = coder->plan.ws_bytes;
            win->d_rows = coder->d_rows;
            for (int s = 0; s < 2; s++) win->groups[s] = win_image[s].size();
            auto up = [](const std::vector<uint32_t> &v, uint32_t **dev) { return v.empty() || sicn::upload(v.data(), v.size() * sizeof(uint32_t), dev); };
            if (!sicn::upload(wrows.data(), wrows.size() * sizeof(CtxWinRow), &win->d_wrows) || !up(win_image[0], &win->d_win_image[0]) ||
                !up(win_image[1], &win->d_win_image[1]))
                rc = SICN_ENOMEM;
        }
    } catch (const std::bad_alloc &) { rc = SICN_ENOMEM; }
    if (rc) {
        sicn_ragged_ctx_window_free(win);
        return rc;
    }
    *out = win;
    return SICN_OK;
}

extern "C" size_t sicn_ragged_ctx_window_workspace_bytes(const sicn_ragged_ctx_window *win) { return win ? (size_t)win->ws_bytes : 0; }

extern "C" int sicn_ragged_ctx_window_decode_async(const sicn_ragged_ctx_window *win, const uint8_t *containers,
                                                   const sicn_codec_status *valid_dev_or_null, const uint8_t *scales, uint8_t *band,
                                                   sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!win || !containers || !scales || !band || !status_dev) return SICN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(band) | reinterpret_cast<uintptr_t>(scales)) & 3) return SICN_EINVAL;   // dword gathers
    if (reinterpret_cast<uintptr_t>(containers) & 1) return SICN_EINVAL;   // the streams are read as 16-bit words (slot offsets are even)
    if (!workspace || workspace_bytes < win->ws_bytes) return SICN_ENOSPC;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return SICN_EINVAL;
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
                       ws, win->d_rows, win->d_wrows, win->d_win_image[0]);
    if (win->groups[1])   // (a window of rows without non-anchors, e.g. of 1 x 1 latents)
        hipLaunchKernelGGL(k_ragged_ctx_decode_window<1>, dim3((unsigned)win->groups[1]), dim3(64 * CTX_WPB_DEC), 0, stream, containers, scales,
                           band, ws, win->d_rows, win->d_wrows, win->d_win_image[1]);
    hipLaunchKernelGGL(k_ragged_ctx_finish_window, dim3(n), dim3(64), 0, stream, (uint32_t *)status_dev, ws, win->d_rows, win->d_wrows);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}
