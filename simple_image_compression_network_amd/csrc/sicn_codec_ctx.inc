// Container mode 4, "rANS-WC": the wavefront rANS of mode 3 with a conditional entropy model — 16 static class tables, the
// class of a symbol given by the hyper-synthesis scale map and, for the non-anchor half of a checkerboard, by its already
// coded anchor neighbours (specification: oracle/sicn_hyper_oracle.c; SURVEY.md §8f row 4; parity UNPINNED — the reference
// has no coder, no hyperprior and no context model).  Textually included at the end of sicn_codec.hip (same translation
// unit: it re-uses k_stats, k_scan, k_compact, k_clear_stats, the exact reciprocal divide and the status conventions).
//
// Everything is asynchronous (device-side statistics / tables / validation, device status words), like the mode-3 pair.
namespace {

// The stages are in k_ctx_body.hpp and, the two step loops, in k_ctx_encode_steps.inc / k_ctx_decode_steps.inc (shared with the ragged
// form, k_ragged_ctx.hip); a kernel here hands its stage image 0's pointers and the strides that img_ptr (blockIdx.y = image)
// advances them by, or resolves them itself in front of an included step loop.
struct CtxStrided {
    size_t s_lat, s_ws, s_slot;
    template <typename T> __device__ __forceinline__ T *lat(T *p) const { return img_ptr(p, s_lat); }
    template <typename T> __device__ __forceinline__ T *ws(T *p) const { return img_ptr(p, s_ws); }
    template <typename T> __device__ __forceinline__ T *slot(T *p) const { return img_ptr(p, s_slot); }
};

// class histograms (+ range check of the scale map)
__global__ __launch_bounds__(256) void k_ctx_hist(const uint8_t *__restrict__ lat_, const uint8_t *__restrict__ scale_, CtxGeom g,
                                                  uint32_t *__restrict__ chist_, uint32_t *__restrict__ meta_, size_t s_lat, size_t s_ws)
{
    ctx_hist_body(CtxStrided{s_lat, s_ws, 0}, lat_, scale_, g, chist_, meta_, blockIdx.x, gridDim.x);
}

// encoder: table_in_ == nullptr, tables come from chist and go to out_; decoder: tables are READ from the container
__global__ __launch_bounds__(1024) void k_ctx_tables(const uint32_t *__restrict__ chist_, const unsigned long long *__restrict__ sums_,
                                                     uint32_t *__restrict__ meta_, uint32_t *__restrict__ tfc_, uint32_t *__restrict__ trcp_,
                                                     uint8_t *__restrict__ tst_, uint8_t *__restrict__ out_, uint32_t *__restrict__ status_,
                                                     CtxGeom g, uint32_t img_w, uint32_t img_h, const uint8_t *__restrict__ table_in_,
                                                     size_t s_ws, size_t s_slot)
{
    ctx_tables_body(CtxStrided{0, s_ws, s_slot}, chist_, sums_, meta_, tfc_, trcp_, tst_, out_, g, img_w, img_h, table_in_);
    (void)status_;
}

// the error word of an image's statistics / table stages -> status[i].error (after every stage has run)
__global__ __launch_bounds__(64) void k_ctx_enc_status(const uint32_t *__restrict__ meta_, const uint32_t *__restrict__ hist_,
                                                       uint32_t *__restrict__ status_, size_t s_ws)
{
    if (threadIdx.x) return;
    status_[2 * blockIdx.y] = ctx_enc_verdict(img_ptr(meta_, s_ws), img_ptr(hist_, s_ws));
}

__global__ __launch_bounds__(64 * CTX_WPB) void k_ctx_encode(const uint8_t *__restrict__ lat_, const uint8_t *__restrict__ scale_, CtxGeom g,
                                                   const uint32_t *__restrict__ tfc_, const uint32_t *__restrict__ trcp_,
                                                   uint8_t *__restrict__ scratch_, uint32_t *__restrict__ lens_, size_t s_lat, size_t s_ws)
{
    const uint8_t *lat = img_ptr(lat_, s_lat), *scale = img_ptr(scale_, s_lat);
    uint8_t *scratch = img_ptr(scratch_, s_ws);
    uint32_t *lens = img_ptr(lens_, s_ws);
    const uint32_t *tfc = img_ptr(tfc_, s_ws), *trcp = img_ptr(trcp_, s_ws);
    const uint32_t grp = blockIdx.x;
#include "k_ctx_encode_steps.inc"
}

// one set per launch (anchors first)
__global__ __launch_bounds__(64 * CTX_WPB_DEC) void k_ctx_decode(const uint8_t *__restrict__ payload_, const uint8_t *__restrict__ scale_, int set,
                                                   CtxGeom g, const uint32_t *__restrict__ tfc_, const uint8_t *__restrict__ tst_,
                                                   const uint32_t *__restrict__ offsets_, uint8_t *__restrict__ lat_,
                                                   uint32_t *__restrict__ meta_, size_t s_slot, size_t s_ws, size_t s_lat)
{
    const uint8_t *payload = img_ptr(payload_, s_slot), *scale = img_ptr(scale_, s_lat), *tst = img_ptr(tst_, s_ws);
    const uint32_t *offsets = img_ptr(offsets_, s_ws), *tfc = img_ptr(tfc_, s_ws);
    uint8_t *lat = img_ptr(lat_, s_lat);
    uint32_t *meta = img_ptr(meta_, s_ws);
    const uint32_t grp = blockIdx.x;
#include "k_ctx_decode_steps.inc"
}

// header of a mode-4 container against the caller's shape (the tables are checked by k_ctx_tables)
__global__ __launch_bounds__(64) void k_ctx_parse(const uint8_t *__restrict__ containers_, const uint32_t *__restrict__ valid_bytes_,
                                                  uint32_t valid_stride, uint32_t *__restrict__ meta_, CtxGeom g, size_t s_slot, size_t s_ws)
{
    const uint32_t valid = valid_bytes_ ? min(valid_bytes_[(size_t)blockIdx.y * valid_stride], (uint32_t)min(s_slot, (size_t)0xFFFFFFFFu))
                                        : (uint32_t)min(s_slot, (size_t)0xFFFFFFFFu);
    ctx_parse_body(CtxStrided{0, s_ws, s_slot}, containers_, valid, meta_, g);
}

}  // namespace

extern "C" size_t sicn_codec_ctx_max_bytes(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c)
{
    const CtxGeom g = ctx_geom(lat_w, lat_h, lat_c);
    const size_t n = (size_t)lat_w * lat_h * lat_c, ns = (size_t)g.nst[0] + g.nst[1];
    return SICN_CODEC_HEADER_BYTES + CTX_TABLE_BYTES + 4 * ns + 2 * n + 256 * ns;
}

extern "C" size_t sicn_codec_ctx_workspace_bytes(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t n_images)
{
    const CtxGeom g = ctx_geom(lat_w, lat_h, lat_c);
    return (size_t)n_images * ctx_ws_bytes(g.nst[0] + g.nst[1]);
}

static int ctx_check_shape(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t n_images)
{
    const unsigned long long n64 = (unsigned long long)lat_w * lat_h * lat_c;
    if (n64 == 0 || n64 > MAX_RANS_SYMBOLS || (lat_c & 3) || n_images > 65535) return SICN_EINVAL;
    return SICN_OK;
}

extern "C" int sicn_codec_ctx_encode_batch_async(const uint8_t *latents, const uint8_t *scales, uint32_t n_images, uint32_t lat_w,
                                                 uint32_t lat_h, uint32_t lat_c, uint32_t img_w, uint32_t img_h, uint8_t *out,
                                                 size_t slot_bytes, sicn_codec_status *status_dev, void *workspace,
                                                 size_t workspace_bytes, void *hip_stream)
{
    if (!latents || !scales || !out || !status_dev) return SICN_EINVAL;
    if (int rc = ctx_check_shape(lat_w, lat_h, lat_c, n_images)) return rc;
    if (n_images == 0) return SICN_OK;
    if (((uintptr_t)latents | (uintptr_t)scales) & 3) return SICN_EINVAL;   // dword gathers
    const CtxGeom g = ctx_geom(lat_w, lat_h, lat_c);
    const uint32_t n = lat_w * lat_h * lat_c, ns = g.nst[0] + g.nst[1];
    if (slot_bytes < sicn_codec_ctx_max_bytes(lat_w, lat_h, lat_c) || (slot_bytes & 1)) return SICN_ENOSPC;
    const size_t ws1 = ctx_ws_bytes(ns);
    if (!workspace || workspace_bytes < ws1 * n_images) return SICN_ENOSPC;
    hipStream_t stream = (hipStream_t)hip_stream;
    CtxWorkspace w;
    ctx_carve(w, workspace, ns, WCAP);
    uint32_t *status = (uint32_t *)status_dev;
    uint8_t *table = out + SICN_CODEC_HEADER_BYTES + CTX_TABLE_BYTES, *payload = table + 4 * (size_t)ns;
    const uint32_t fixed = (uint32_t)(SICN_CODEC_HEADER_BYTES + CTX_TABLE_BYTES + 4 * (size_t)ns);
    hipLaunchKernelGGL(k_clear_stats, dim3(1, n_images), dim3(64), 0, stream, w.hist, ws1);
    HIP_TRY(hipMemset2DAsync(w.chist, ws1, 0, NCLS * 128 * 4, n_images, stream));
    hipLaunchKernelGGL(k_stats, dim3(stats_blocks(n), n_images), dim3(256), 0, stream, latents, (uint8_t *)workspace, stats_batch(n, n, ws1));
    hipLaunchKernelGGL(k_ctx_hist, dim3(ctx_hist_blocks(n), n_images), dim3(256), 0, stream, latents, scales, g, w.chist,
                       w.meta, (size_t)n, ws1);
    hipLaunchKernelGGL(k_ctx_tables, dim3(1, n_images), dim3(1024), 0, stream, w.chist, w.sums, w.meta, w.tfc, w.trcp, w.tst, out, status,
                       g, img_w, img_h, (const uint8_t *)nullptr, ws1, slot_bytes);
    hipLaunchKernelGGL(k_ctx_enc_status, dim3(1, n_images), dim3(64), 0, stream, w.meta, w.hist, status, ws1);
    hipLaunchKernelGGL(k_ctx_encode, dim3((ns + CTX_WPB - 1) / CTX_WPB, n_images), dim3(64 * CTX_WPB), 0, stream, latents, scales, g, w.tfc, w.trcp, w.scratch, w.lens,
                       (size_t)n, ws1);
    hipLaunchKernelGGL(k_scan, dim3(1, n_images), dim3(1024), 0, stream, w.lens, (const uint8_t *)nullptr, ns, w.offsets, table,
                       out + 40, ws1, slot_bytes, 0xFFFFFFFFu, (uint32_t *)nullptr, status, fixed);
    hipLaunchKernelGGL(k_compact, dim3(ns, n_images), dim3(256), 0, stream, w.scratch, w.lens, w.offsets, payload, WCAP, ws1, slot_bytes);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_codec_ctx_decode_batch_async(const uint8_t *containers, size_t slot_bytes, const sicn_codec_status *valid_dev_or_null,
                                                 const uint8_t *scales, uint32_t n_images, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c,
                                                 uint8_t *latents, sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes,
                                                 void *hip_stream)
{
    if (!containers || !scales || !latents || !status_dev || (slot_bytes & 1)) return SICN_EINVAL;
    if (int rc = ctx_check_shape(lat_w, lat_h, lat_c, n_images)) return rc;
    if (n_images == 0) return SICN_OK;
    if (((uintptr_t)latents | (uintptr_t)scales) & 3) return SICN_EINVAL;
    const CtxGeom g = ctx_geom(lat_w, lat_h, lat_c);
    const uint32_t n = lat_w * lat_h * lat_c, ns = g.nst[0] + g.nst[1];
    const size_t ws1 = ctx_ws_bytes(ns);
    if (!workspace || workspace_bytes < ws1 * n_images) return SICN_ENOSPC;
    hipStream_t stream = (hipStream_t)hip_stream;
    CtxWorkspace w;
    ctx_carve(w, workspace, ns, 0);
    const uint8_t *tables = containers + SICN_CODEC_HEADER_BYTES, *table = tables + CTX_TABLE_BYTES, *payload = table + 4 * (size_t)ns;
    hipLaunchKernelGGL(k_ctx_parse, dim3(1, n_images), dim3(64), 0, stream, containers,
                       valid_dev_or_null ? &valid_dev_or_null->bytes : (const uint32_t *)nullptr, 2u, w.meta, g, slot_bytes, ws1);
    hipLaunchKernelGGL(k_ctx_tables, dim3(1, n_images), dim3(1024), 0, stream, (const uint32_t *)nullptr, (const unsigned long long *)nullptr,
                       w.meta, w.tfc, w.trcp, w.tst, (uint8_t *)nullptr, (uint32_t *)nullptr, g, 0u, 0u, tables, ws1, slot_bytes);
    hipLaunchKernelGGL(k_scan, dim3(1, n_images), dim3(1024), 0, stream, (const uint32_t *)nullptr, table, ns, w.offsets,
                       (uint8_t *)nullptr, (uint8_t *)nullptr, ws1, slot_bytes, WCAP, w.meta + 3, (uint32_t *)nullptr, 0u,
                       (const uint32_t *)w.meta);
    // a non-anchor's class reads its neighbours' bytes whatever they hold: start from zeros so that a rejected container
    // cannot make the result depend on what the buffer held before
    HIP_TRY(hipMemsetAsync(latents, 0, (size_t)n * n_images, stream));
    for (int set = 0; set < 2; set++)
        if (g.nst[set])
            hipLaunchKernelGGL(k_ctx_decode, dim3((g.nst[set] + CTX_WPB_DEC - 1) / CTX_WPB_DEC, n_images), dim3(64 * CTX_WPB_DEC), 0, stream, payload, scales, set, g, w.tfc, w.tst,
                               w.offsets, latents, w.meta, slot_bytes, ws1, (size_t)n);
    hipLaunchKernelGGL(k_stats, dim3(stats_blocks(n), n_images), dim3(256), 0, stream, latents, (uint8_t *)workspace, stats_batch(n, n, ws1));
    hipLaunchKernelGGL(k_dec_finish, dim3(1, n_images), dim3(64), 0, stream, w.meta, w.sums, w.offsets, (uint32_t *)status_dev, n, ns, ws1);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}
