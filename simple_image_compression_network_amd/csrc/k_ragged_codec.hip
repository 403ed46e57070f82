// Ragged latent coder (include/sicn_ragged_codec.h): the rANS-W stages of k_codec_body.hpp over n latents of n different shapes, three
// launches per encode and two per decode for the whole batch.  The stage bodies are the uniform coder's (sicn_codec.hip); what is
// new is how a workgroup finds its image.
//
// Grid: flat over work items — k_ragged_stats: the statistics rows of all images (min(max(n_i / 16384, 1), STAT_ROWS) each, the
// uniform coder's rule); encode, compaction and decode: the streams of all images; the decoder's finish: one workgroup per image.
// Two kinds of table, built on the host at creation:
//   row_image[row], stream_image[stream] : the image a work item belongs to — ONE load resolves item -> image
//   rows[image]                          : CoderRow (k_codec_body.hpp, with enc_image() / dec_image()), the image's sizes, its first
//                                          work items and its 64-bit byte offsets in the latent tensor, the slot buffer and the workspace
// Both loads are wave-uniform (they depend on blockIdx.x only) and stay in scalar registers.  The workspace block of an image is
// what carve() gives for (ns_i, wstream_cap(wss_i)), the same function the uniform coder calls on the host.
#include <vector>

#include "../../include/sicn_ragged_codec.h"
#include "device_table.hpp"
#include "k_codec_body.hpp"
#include "sicn_internal.h"

namespace {

__global__ __launch_bounds__(256) void k_ragged_stats(const uint8_t *__restrict__ latents, uint8_t *__restrict__ workspace,
                                                      const CoderRow *__restrict__ rows, const uint32_t *__restrict__ row_image)
{
    const uint32_t img = uni(row_image[blockIdx.x]);
    const CoderRow r = load_row(rows, img);
    const uint32_t local = blockIdx.x - r.first_row;
    Workspace w;
    carve(w, workspace + r.ws_off, r.ns, wstream_cap(r.wss));
    stats_body(latents + r.lat_off, r.n, w.hist, w.sums, w.rows + (size_t)local * STAT_ROW_WORDS, local, r.n_rows);
}

__global__ __launch_bounds__(64) void k_ragged_encode(const uint8_t *__restrict__ latents, uint8_t *__restrict__ containers,
                                                      uint32_t *__restrict__ status, uint8_t *__restrict__ workspace,
                                                      const CoderRow *__restrict__ rows, const uint32_t *__restrict__ stream_image)
{
    const uint32_t img = uni(stream_image[blockIdx.x]);
    const CoderRow r = load_row(rows, img);
    ransw_encode_body(enc_image(r, latents, containers, status, workspace, img), blockIdx.x - r.first_stream);
}

__global__ __launch_bounds__(256) void k_ragged_compact(uint8_t *__restrict__ containers, uint32_t *__restrict__ status,
                                                        uint8_t *__restrict__ workspace, const CoderRow *__restrict__ rows,
                                                        const uint32_t *__restrict__ stream_image)
{
    const uint32_t img = uni(stream_image[blockIdx.x]);
    const CoderRow r = load_row(rows, img);
    compact_self_body(enc_image(r, nullptr, containers, status, workspace, img), blockIdx.x - r.first_stream, wstream_cap(r.wss),
                      (uint32_t)(SICN_CODEC_HEADER_BYTES + 256) + 4 * r.ns);
}

template <bool BIGTAB>
__global__ __launch_bounds__(64) void k_ragged_decode(const uint8_t *__restrict__ containers, const uint32_t *__restrict__ valid,
                                                      uint8_t *__restrict__ latents, uint8_t *__restrict__ workspace,
                                                      const CoderRow *__restrict__ rows, const uint32_t *__restrict__ stream_image)
{
    const uint32_t img = uni(stream_image[blockIdx.x]);
    const CoderRow r = load_row(rows, img);
    ransw_decode_body<BIGTAB>(dec_image(r, containers, valid, latents, nullptr, workspace, img), blockIdx.x - r.first_stream, 1);
}

__global__ __launch_bounds__(256) void k_ragged_dec_finish(const uint8_t *__restrict__ containers, const uint32_t *__restrict__ valid,
                                                           uint32_t *__restrict__ status, uint8_t *__restrict__ workspace,
                                                           const CoderRow *__restrict__ rows)
{
    const uint32_t img = blockIdx.x;
    const CoderRow r = load_row(rows, img);
    dec_finish_self_body(dec_image(r, containers, valid, nullptr, status, workspace, img));
}

// ---- the layout: pure host --------------------------------------------------------------------------------------------------
constexpr uint64_t RAGGED_MAX_STREAMS = 0x7fffffffull;   // fewer streams than this in all (grid.x)

struct Plan {
    std::vector<CoderRow> rows;
    uint64_t lat_bytes = 0, slot_bytes = 0, ws_bytes = 0, streams = 0, stat_rows = 0;
};

// keep_rows = false: totals only (nothing is allocated)
int plan_coder(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *wss_or_null, const uint32_t *img_w,
               const uint32_t *img_h, int n_images, bool keep_rows, sicn_ragged_codec_image *images, Plan *p)
{
    if (!lat_w || !lat_h || n_images < 1 || lat_c < 1) return SICN_EINVAL;
    if (keep_rows) p->rows.reserve((size_t)n_images);
    for (int i = 0; i < n_images; i++) {
        const uint32_t wss = wss_or_null ? wss_or_null[i] : WSS;
        if (lat_w[i] < 1 || lat_h[i] < 1 || !wstream_ok(wss)) return SICN_EINVAL;
        const uint64_t most = (uint64_t)SELF_SCAN_MAX * wss;            // <= 2^25: the products below cannot wrap
        const uint64_t positions = (uint64_t)lat_w[i] * lat_h[i];
        if (positions > most || positions * lat_c > most) return SICN_EINVAL;
        const uint32_t n = (uint32_t)(positions * lat_c), ns = (n + wss - 1) / wss;
        Workspace w;
        CoderRow r{};
        r.lat_off = p->lat_bytes;
        r.slot_off = p->slot_bytes;
        r.ws_off = p->ws_bytes;
        r.n = n; r.ns = ns; r.wss = wss;
        r.slot_cap = (uint32_t)align_up(SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)ns + 2 * (size_t)n + 256 * (size_t)ns, 16);   // sicn_codec_max_bytes_sl
        r.lat_w = lat_w[i]; r.lat_h = lat_h[i]; r.lat_c = lat_c;
        r.img_w = img_w ? img_w[i] : 0; r.img_h = img_h ? img_h[i] : 0;
        r.first_stream = (uint32_t)p->streams;
        r.first_row = (uint32_t)p->stat_rows;
        r.n_rows = stat_rows(n);
        p->lat_bytes += n;
        p->slot_bytes += r.slot_cap;
        p->ws_bytes += align_up(carve(w, nullptr, ns, wstream_cap(wss)), 256);
        p->streams += ns;
        p->stat_rows += r.n_rows;
        if (p->streams >= RAGGED_MAX_STREAMS) return SICN_EINVAL;
        if (images) images[i] = sicn_ragged_codec_image{r.lat_off, r.slot_off, r.ws_off, r.slot_cap, n, ns, wss};
        if (keep_rows) p->rows.push_back(r);
    }
    return SICN_OK;
}

}  // namespace

struct sicn_ragged_coder {
    int n_images = 0;
    Plan plan;
    sicn::DeviceTable<CoderRow> d_rows;             // [n_images]
    sicn::DeviceTable<uint32_t> d_stream_image;     // [streams]
    sicn::DeviceTable<uint32_t> d_row_image;        // [stat_rows]
};

extern "C" int sicn_ragged_codec_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                                        int n_images, sicn_ragged_codec_image *images_or_null, uint64_t totals[3])
{
    Plan p;
    if (int rc = plan_coder(lat_w, lat_h, lat_c, stream_symbols_or_null, nullptr, nullptr, n_images, false, images_or_null, &p)) return rc;
    if (totals) {
        totals[0] = p.lat_bytes;
        totals[1] = p.slot_bytes;
        totals[2] = p.ws_bytes;
    }
    return SICN_OK;
}

extern "C" void sicn_ragged_coder_free(sicn_ragged_coder *coder) { delete coder; }

extern "C" int sicn_ragged_coder_create(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                                        const uint32_t *image_w_or_null, const uint32_t *image_h_or_null, int n_images,
                                        sicn_ragged_coder **out)
{
    return sicn::make_object(out, [&](sicn_ragged_coder &coder) {
        if (int rc = plan_coder(lat_w, lat_h, lat_c, stream_symbols_or_null, image_w_or_null, image_h_or_null, n_images, true, nullptr, &coder.plan))
            return rc;
        if (int rc = sicn::chip_geom(nullptr)) return rc;       // no device, or not a gfx950 one
        coder.n_images = n_images;
        sicn::ItemMap stream_image, row_image;
        for (int i = 0; i < n_images; i++) {
            const CoderRow &r = coder.plan.rows[(size_t)i];
            stream_image.add(r.ns, (uint32_t)i);
            row_image.add(r.n_rows, (uint32_t)i);
        }
        const bool ok = coder.d_rows.upload(coder.plan.rows) && stream_image.upload(coder.d_stream_image) && row_image.upload(coder.d_row_image);
        return ok ? SICN_OK : SICN_ENOMEM;
    });
}

// what the window decoder (k_ragged_window.hip) builds on: the coder's rows, on the host and on the device
void sicn::ragged_coder_view(const sicn_ragged_coder *coder, RaggedCoderView *v)
{
    v->n_images = coder->n_images;
    v->rows_host = coder->plan.rows.data();
    v->d_rows = coder->d_rows.get();
    v->row_bytes = sizeof(CoderRow);
    v->ws_bytes = coder->plan.ws_bytes;
}

extern "C" size_t sicn_ragged_coder_workspace_bytes(const sicn_ragged_coder *coder) { return coder ? (size_t)coder->plan.ws_bytes : 0; }

extern "C" int sicn_ragged_coder_encode_async(const sicn_ragged_coder *coder, const uint8_t *latents, uint8_t *containers,
                                              sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!coder || !latents || !containers || !status_dev) return SICN_EINVAL;
    if (int rc = sicn::workspace_rc(workspace, workspace_bytes, coder->plan.ws_bytes)) return rc;
    if (int rc = sicn::chip_geom(nullptr)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    uint32_t *status = (uint32_t *)status_dev;
    const unsigned streams = (unsigned)coder->plan.streams, stat_rows = (unsigned)coder->plan.stat_rows;
    // the uniform coder's three stages (sicn_codec_encode_batch_async_sl, self-scanning form): statistics in rows -> streams, every
    // wave making the frequency table itself and stream 0's wave of an image writing its header -> compaction with its own scan
    hipLaunchKernelGGL(k_ragged_stats, dim3(stat_rows), dim3(256), 0, stream, latents, ws, coder->d_rows.get(), coder->d_row_image.get());
    hipLaunchKernelGGL(k_ragged_encode, dim3(streams), dim3(64), 0, stream, latents, containers, status, ws, coder->d_rows.get(),
                       coder->d_stream_image.get());
    hipLaunchKernelGGL(k_ragged_compact, dim3(streams), dim3(256), 0, stream, containers, status, ws, coder->d_rows.get(),
                       coder->d_stream_image.get());
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_ragged_coder_decode_async(const sicn_ragged_coder *coder, const uint8_t *containers,
                                              const sicn_codec_status *valid_dev_or_null, uint8_t *latents, sicn_codec_status *status_dev,
                                              void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!coder || !containers || !latents || !status_dev) return SICN_EINVAL;
    if (int rc = sicn::workspace_rc(workspace, workspace_bytes, coder->plan.ws_bytes)) return rc;
    sicn::ChipGeom chip;
    if (int rc = sicn::chip_geom(&chip)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    const uint32_t *valid = (const uint32_t *)valid_dev_or_null;
    const unsigned streams = (unsigned)coder->plan.streams;
    // the latency form (one 16 KB table) while all waves of the BATCH fit the chip at five per CU, as in the uniform decoder
    if (coder->plan.streams <= 5ull * (unsigned)chip.n_cu)
        hipLaunchKernelGGL(k_ragged_decode<true>, dim3(streams), dim3(64), 0, stream, containers, valid, latents, ws, coder->d_rows.get(),
                           coder->d_stream_image.get());
    else
        hipLaunchKernelGGL(k_ragged_decode<false>, dim3(streams), dim3(64), 0, stream, containers, valid, latents, ws, coder->d_rows.get(),
                           coder->d_stream_image.get());
    hipLaunchKernelGGL(k_ragged_dec_finish, dim3((unsigned)coder->n_images), dim3(256), 0, stream, containers, valid, (uint32_t *)status_dev,
                       ws, coder->d_rows.get());
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}
