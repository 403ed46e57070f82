// Random access inside an image (include/sicn_ragged_window.h): the window decoder — the rANS-W decode stage of k_codec_body.hpp over
// a SELECTION of every image's streams, two launches for the batch — and the cut of a rectangle out of every image of a ragged
// tensor, one launch.  A translation unit of its own: the kernels of k_ragged_codec.hip and sicn_codec.hip keep their code as it is.
//
// Window decoder.  Grid of k_ragged_decode_window: flat over the selected streams of all images.  Tables:
//   stream_image[item] : the image of a selected stream — ONE load resolves item -> image
//   rows[image]        : the CODER's CoderRow table (the window is made over an existing sicn_ragged_coder and reads its device copy)
//   wrows[image]       : WinRow, the image's first selected stream, its first item, and where its band lies
// All three loads are wave-uniform.  ransw_decode_body runs unchanged with the stream's REAL index st — it sums the length table up
// to st and writes its symbols at lat + st * wss — and is handed a latent pointer biased by -first_stream * wss, so the symbols land
// in the band.  Its per-stream words (verdict, checksum sums) are indexed by st too, which is why the workspace is the full coder's.
// k_ragged_dec_finish_window: one workgroup per image, dec_finish_window_body.
//
// Cut.  The one rectangle copy of the ragged family; the crop of sicn_ragged_hyper.h (k_ragged.hip) is this cut at the corner.  The
// pattern of k_any_ragged: a work item of CUT_ROWS destination rows (the image's last item: the rest), the image through two
// wave-uniform loads,
//   item_image[item] : the image of an item
//   rows[image]      : CutRow { source / destination row bytes, destination rows, first item, vec, 64-bit offsets in src and dst }
// The row's src_off leads to the rectangle's first byte (window_host.hpp), so a rectangle at any offset costs what a corner does.
#include <new>
#include <vector>

#include "../../include/sicn_ragged_window.h"
#include "device_table.hpp"
#include "k_codec_body.hpp"
#include "sicn_internal.h"
#include "window_host.hpp"

namespace {

struct WinRow {
    uint64_t lat_bias;                  // band_offset - first_stream * wss, modulo 2^64: added to the band tensor's address
    uint32_t first_stream, end_stream;  // the selected streams, in the image's own numbering
    uint32_t first_item;                // the image's first work item in the flat grid
    uint32_t symbols;                   // what the selected streams hold
};

template <bool BIGTAB>
__global__ __launch_bounds__(64) void k_ragged_decode_window(const uint8_t *__restrict__ containers, const uint32_t *__restrict__ valid,
                                                             uint8_t *__restrict__ band, uint8_t *__restrict__ workspace,
                                                             const CoderRow *__restrict__ rows, const WinRow *__restrict__ wrows,
                                                             const uint32_t *__restrict__ stream_image)
{
    const uint32_t img = uni(stream_image[blockIdx.x]);
    const CoderRow r = load_row(rows, img);
    const WinRow *w = wrows + img;
    const uint32_t st = blockIdx.x - uni(w->first_item) + uni(w->first_stream);
    DecImage im = dec_image(r, containers, valid, band, nullptr, workspace, img);
    im.lat = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(band) + uni(w->lat_bias));
    ransw_decode_body<BIGTAB>(im, st, 1);
}

__global__ __launch_bounds__(256) void k_ragged_dec_finish_window(const uint8_t *__restrict__ containers, const uint32_t *__restrict__ valid,
                                                                  uint32_t *__restrict__ status, uint8_t *__restrict__ workspace,
                                                                  const CoderRow *__restrict__ rows, const WinRow *__restrict__ wrows)
{
    const uint32_t img = blockIdx.x;
    const CoderRow r = load_row(rows, img);
    const WinRow *w = wrows + img;
    dec_finish_window_body(dec_image(r, containers, valid, nullptr, status, workspace, img), uni(w->first_stream), uni(w->end_stream),
                           uni(w->symbols));
}

using sicn_window::CutRow;
constexpr int CUT_ROWS = sicn_window::CUT_ROWS;

// `vec` (per image, host-made): both row pitches, the rectangle's byte offset and the destination offset are multiples of 16;
// `ptr16` (per launch): so are both base pointers.  Then a row is copied as uint4, otherwise byte by byte.
__global__ __launch_bounds__(256) void k_ragged_cut(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const CutRow *__restrict__ rows,
                                                    const uint32_t *__restrict__ item_image, int ptr16)
{
    const uint32_t item = blockIdx.x;
    const uint32_t img = uni(item_image[item]);
    const CutRow *row = rows + img;
    const uint32_t src_row = uni(row->src_row), dst_row = uni(row->dst_row), dst_h = uni(row->dst_h);
    const uint32_t y0 = (item - uni(row->first_item)) * (uint32_t)CUT_ROWS;
    const int vec = (int)uni(row->vec) & ptr16;
    const uint64_t src_off = uni((uint64_t)row->src_off), dst_off = uni((uint64_t)row->dst_off);
    if (y0 >= dst_h) return;                                  // cannot happen with the host's tables
    const uint32_t n_rows = dst_h - y0 < (uint32_t)CUT_ROWS ? dst_h - y0 : (uint32_t)CUT_ROWS;
    // one image's tensor is < 2^31 bytes (host check), so every index below fits 32 bits
    const uint8_t *s = src + src_off + (size_t)y0 * src_row;
    uint8_t *d = dst + dst_off + (size_t)y0 * dst_row;
    if (vec) {
        const uint32_t q_row = dst_row / 16, total = n_rows * q_row;
        for (uint32_t i = threadIdx.x; i < total; i += 256) {
            const uint32_t r = i / q_row, q = i - r * q_row;
            reinterpret_cast<uint4 *>(d + (size_t)r * dst_row)[q] = reinterpret_cast<const uint4 *>(s + (size_t)r * src_row)[q];
        }
    } else {
        const uint32_t total = n_rows * dst_row;
        for (uint32_t i = threadIdx.x; i < total; i += 256) {
            const uint32_t r = i / dst_row, b = i - r * dst_row;
            d[(size_t)r * dst_row + b] = s[(size_t)r * src_row + b];
        }
    }
}

}  // namespace

// ---- the plan and the layouts: pure host ---------------------------------------------------------------------------------------
extern "C" int sicn_ragged_roi_plan(int n_up_layers, int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, const sicn_ragged_rect *rect,
                                    sicn_ragged_roi *out)
{
    return sicn_window::roi_plan(n_up_layers, image_w, image_h, lat_w, lat_h, rect, out);
}

extern "C" int sicn_ragged_window_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                                         const uint32_t *r0, const uint32_t *rh, int n_images, sicn_ragged_window_image *images_or_null,
                                         uint64_t totals[2])
{
    uint64_t coder[3] = {0, 0, 0}, band = 0;
    if (int rc = sicn_ragged_codec_layout(lat_w, lat_h, lat_c, stream_symbols_or_null, n_images, nullptr, coder)) return rc;
    if (int rc = sicn_window::window_layout(lat_w, lat_h, lat_c, stream_symbols_or_null, r0, rh, n_images, images_or_null, &band, nullptr)) return rc;
    if (totals) {
        totals[0] = band;
        totals[1] = coder[2];
    }
    return SICN_OK;
}

// ---- the window decoder ----------------------------------------------------------------------------------------------------------
struct sicn_ragged_window {
    int n_images = 0;
    uint64_t streams = 0, ws_bytes = 0;
    const CoderRow *d_rows = nullptr;       // the coder's
    sicn::DeviceTable<WinRow> d_wrows;              // [n_images]
    sicn::DeviceTable<uint32_t> d_stream_image;     // [streams]
};

extern "C" void sicn_ragged_window_free(sicn_ragged_window *win) { delete win; }

extern "C" int sicn_ragged_window_create(const sicn_ragged_coder *coder, const uint32_t *r0, const uint32_t *rh, sicn_ragged_window **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    if (!coder || !r0 || !rh) return SICN_EINVAL;
    sicn::RaggedCoderView v;
    sicn::ragged_coder_view(coder, &v);
    if (v.row_bytes != sizeof(CoderRow) || v.n_images < 1) return SICN_EINVAL;
    const CoderRow *rows = (const CoderRow *)v.rows_host;
    return sicn::make_object(out, [&](sicn_ragged_window &win) {
        std::vector<WinRow> wrows((size_t)v.n_images);
        sicn::ItemMap stream_image;
        uint64_t at = 0;
        for (int i = 0; i < v.n_images; i++) {
            const CoderRow &r = rows[i];
            sicn_ragged_window_image im;
            if (int rc = sicn_window::band_of(r.lat_w, r.lat_h, r.lat_c, r.wss, r0[i], rh[i], at, &im)) return rc;
            // the items are <= the coder's streams, which fit a grid
            const uint32_t first_item = stream_image.add(im.end_stream - im.first_stream, (uint32_t)i);
            wrows[(size_t)i] = WinRow{at - (uint64_t)im.first_stream * r.wss, im.first_stream, im.end_stream, first_item, im.band_bytes};
            at += sicn_window::a16(im.band_bytes);
        }
        if (int rc = sicn::chip_geom(nullptr)) return rc;       // no device, or not a gfx950 one
        win.n_images = v.n_images;
        win.streams = stream_image.size();
        win.ws_bytes = v.ws_bytes;
        win.d_rows = (const CoderRow *)v.d_rows;
        return win.d_wrows.upload(wrows) && stream_image.upload(win.d_stream_image) ? SICN_OK : SICN_ENOMEM;
    });
}

extern "C" size_t sicn_ragged_window_workspace_bytes(const sicn_ragged_window *win) { return win ? (size_t)win->ws_bytes : 0; }

extern "C" int sicn_ragged_window_decode_async(const sicn_ragged_window *win, const uint8_t *containers,
                                               const sicn_codec_status *valid_dev_or_null, uint8_t *band, sicn_codec_status *status_dev,
                                               void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!win || !containers || !band || !status_dev) return SICN_EINVAL;
    if (int rc = sicn::workspace_rc(workspace, workspace_bytes, win->ws_bytes)) return rc;
    sicn::ChipGeom chip;
    if (int rc = sicn::chip_geom(&chip)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    const uint32_t *valid = (const uint32_t *)valid_dev_or_null;
    const unsigned streams = (unsigned)win->streams;
    // the latency form (one 16 KB table) while all waves of the SELECTION fit the chip at five per CU, the full decoder's rule
    if (win->streams <= 5ull * (unsigned)chip.n_cu)
        hipLaunchKernelGGL(k_ragged_decode_window<true>, dim3(streams), dim3(64), 0, stream, containers, valid, band, ws, win->d_rows,
                           win->d_wrows.get(), win->d_stream_image.get());
    else
        hipLaunchKernelGGL(k_ragged_decode_window<false>, dim3(streams), dim3(64), 0, stream, containers, valid, band, ws, win->d_rows,
                           win->d_wrows.get(), win->d_stream_image.get());
    hipLaunchKernelGGL(k_ragged_dec_finish_window, dim3((unsigned)win->n_images), dim3(256), 0, stream, containers, valid,
                       (uint32_t *)status_dev, ws, win->d_rows, win->d_wrows.get());
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

// ---- the cut ----------------------------------------------------------------------------------------------------------------------
struct sicn_ragged_cut {
    int n_images = 0;
    unsigned items = 0;
    sicn::DeviceTable<CutRow> d_rows;               // [n_images]
    sicn::DeviceTable<uint32_t> d_item_image;       // [items]
};

namespace {

struct CutTables {
    std::vector<CutRow> rows;               // [n_images]
    std::vector<int64_t> first_item;        // [n_images + 1]
    std::vector<int64_t> image_off;         // [n_images]
    int64_t totals[2] = {0, 0};
};

// cut_plan's first check in front of the arrays it fills, so that nothing is sized by an n_images it would refuse
int cut_tables(const int32_t *src_w, const int32_t *src_h, const sicn_ragged_rect *rects, int channels, const uint64_t *src_offset_or_null,
               int n_images, CutTables *t)
{
    if (!src_w || !src_h || !rects || n_images < 1 || channels < 1) return SICN_EINVAL;
    try {
        t->rows.resize((size_t)n_images);
        t->first_item.resize((size_t)n_images + 1);
        t->image_off.resize((size_t)n_images);
    } catch (const std::bad_alloc &) { return SICN_ENOMEM; }
    return sicn_window::cut_plan(src_w, src_h, rects, channels, src_offset_or_null, n_images, t->rows.data(), t->first_item.data(),
                                 t->image_off.data(), t->totals);
}

}  // namespace

int sicn::ragged_cut_layout(const int32_t *src_w, const int32_t *src_h, const sicn_ragged_rect *rects, int channels,
                            const uint64_t *src_offset_or_null, int n_images, int image, int64_t out[4])
{
    if (!out) return SICN_EINVAL;
    CutTables t;
    if (int rc = cut_tables(src_w, src_h, rects, channels, src_offset_or_null, n_images, &t)) return rc;
    if (image < 0 || image >= n_images) return SICN_EINVAL;
    out[0] = t.image_off[(size_t)image];
    out[1] = t.rows[(size_t)image].dst_off;
    out[2] = t.totals[0];
    out[3] = t.totals[1];
    return SICN_OK;
}

int sicn::ragged_cut_create(const int32_t *src_w, const int32_t *src_h, const sicn_ragged_rect *rects, int channels,
                            const uint64_t *src_offset_or_null, int n_images, sicn_ragged_cut **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    CutTables t;
    if (int rc = cut_tables(src_w, src_h, rects, channels, src_offset_or_null, n_images, &t)) return rc;
    if (int rc = chip_geom(nullptr)) return rc;      // no device, or not a gfx950 one
    return make_object(out, [&](sicn_ragged_cut &cut) {
        cut.n_images = n_images;
        cut.items = (unsigned)t.first_item[(size_t)n_images];
        ItemMap map;
        for (int i = 0; i < n_images; i++) map.add((size_t)(t.first_item[(size_t)i + 1] - t.first_item[(size_t)i]), (uint32_t)i);
        return cut.d_rows.upload(t.rows) && map.upload(cut.d_item_image) ? SICN_OK : SICN_ENOMEM;
    });
}

int sicn::ragged_cut_run(const sicn_ragged_cut *cut, const uint8_t *src, uint8_t *dst, void *hip_stream)
{
    if (!cut || !src || !dst) return SICN_EINVAL;
    if (int rc = chip_geom(nullptr)) return rc;
    return ragged_cut_launch(cut->d_rows.get(), cut->d_item_image.get(), cut->items, src, dst, hip_stream);
}

int sicn::ragged_cut_launch(const void *d_rows, const uint32_t *d_item_image, unsigned items, const uint8_t *src, uint8_t *dst, void *hip_stream)
{
    const int ptr16 = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    hipLaunchKernelGGL(k_ragged_cut, dim3(items), dim3(256), 0, (hipStream_t)hip_stream, src, dst, (const CutRow *)d_rows, d_item_image, ptr16);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_ragged_cut_layout(const int32_t *src_w, const int32_t *src_h, const sicn_ragged_rect *rects, int channels,
                                      const uint64_t *src_offset_or_null, int n_images, int image, int64_t out[4])
{
    return sicn::ragged_cut_layout(src_w, src_h, rects, channels, src_offset_or_null, n_images, image, out);
}

extern "C" int sicn_ragged_cut_create(const int32_t *src_w, const int32_t *src_h, const sicn_ragged_rect *rects, int channels,
                                      const uint64_t *src_offset_or_null, int n_images, sicn_ragged_cut **out)
{
    return sicn::ragged_cut_create(src_w, src_h, rects, channels, src_offset_or_null, n_images, out);
}

extern "C" void sicn_ragged_cut_free(sicn_ragged_cut *cut) { delete cut; }

extern "C" int sicn_ragged_cut_run(const sicn_ragged_cut *cut, const uint8_t *src, uint8_t *dst, void *hip_stream)
{
    return sicn::ragged_cut_run(cut, src, dst, hip_stream);
}
