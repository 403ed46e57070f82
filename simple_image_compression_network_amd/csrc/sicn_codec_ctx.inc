// Container mode 4, "rANS-WC": the wavefront rANS of mode 3 with a conditional entropy model — 16 static class tables, the
// class of a symbol given by the hyper-synthesis scale map and, for the non-anchor half of a checkerboard, by its already
// coded anchor neighbours (specification: oracle/sicn_hyper_oracle.c; SURVEY.md §8f row 4; parity UNPINNED — the reference
// has no coder, no hyperprior and no context model).  Textually included at the end of sicn_codec.hip (same translation
// unit: it re-uses k_clear_stats and k_stats on the statistics block, the exact reciprocal divide and the status conventions).
//
// Everything is asynchronous (device-side statistics / tables / validation, device status words), like the mode-3 pair.
namespace {

// The stages are in k_ctx_body.hpp (shared with the ragged form, k_ragged_ctx.hip).  A kernel here gets the batch as a CtxBatch by
// value: batch_row() makes this image's row (blockIdx.y = image), ctx_image() resolves it, the stage gets blockIdx.x.
__global__ __launch_bounds__(256) void k_ctx_hist(const uint8_t *__restrict__ latents, const uint8_t *__restrict__ scales,
                                                  uint8_t *__restrict__ workspace, CtxBatch b)
{
    ctx_hist_body(ctx_image(batch_row(b), latents, scales, nullptr, workspace), blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(1024) void k_ctx_tables(uint8_t *__restrict__ containers, uint8_t *__restrict__ workspace, CtxBatch b, int dec)
{
    ctx_tables_body(ctx_image(batch_row(b), nullptr, nullptr, containers, workspace), dec);
}

// the error word of an image's statistics / table stages -> status[i].error (after every stage has run)
__global__ __launch_bounds__(64) void k_ctx_enc_status(uint32_t *__restrict__ status, uint8_t *__restrict__ workspace, CtxBatch b)
{
    if (threadIdx.x) return;
    const CtxImage im = ctx_image(batch_row(b), nullptr, nullptr, nullptr, workspace);
    status[2 * blockIdx.y] = ctx_enc_verdict(im.w.meta, im.w.hist);
}

__global__ __launch_bounds__(64 * CTX_WPB) void k_ctx_encode(const uint8_t *__restrict__ latents, const uint8_t *__restrict__ scales,
                                                             uint8_t *__restrict__ workspace, CtxBatch b)
{
    ctx_encode_body(ctx_image(batch_row(b), latents, scales, nullptr, workspace), blockIdx.x);
}

// one set per launch (anchors first)
template <int SET>
__global__ __launch_bounds__(64 * CTX_WPB_DEC) void k_ctx_decode(const uint8_t *__restrict__ containers, const uint8_t *__restrict__ scales,
                                                                 uint8_t *__restrict__ latents, uint8_t *__restrict__ workspace, CtxBatch b)
{
    const CtxImage im = ctx_image(batch_row(b), latents, scales, containers, workspace);
    ctx_decode_body<SET>(im, blockIdx.x * CTX_WPB_DEC, im.g.nst[SET]);
}

// valid: a sicn_codec_status array or nullptr
__global__ __launch_bounds__(64) void k_ctx_parse(const uint8_t *__restrict__ containers, const uint32_t *__restrict__ valid,
                                                  uint8_t *__restrict__ workspace, CtxBatch b)
{
    ctx_parse_body(ctx_image(batch_row(b), nullptr, nullptr, containers, workspace), valid, blockIdx.y);
}

// status: the encoder's (the decoder passes nullptr)
__global__ __launch_bounds__(1024) void k_ctx_scan(uint8_t *__restrict__ containers, uint32_t *__restrict__ status,
                                                   uint8_t *__restrict__ workspace, CtxBatch b, int dec)
{
    ctx_scan_body(ctx_image(batch_row(b), nullptr, nullptr, containers, workspace), status, blockIdx.y, dec);
}

__global__ __launch_bounds__(256) void k_ctx_compact(uint8_t *__restrict__ containers, uint8_t *__restrict__ workspace, CtxBatch b)
{
    ctx_compact_body(ctx_image(batch_row(b), nullptr, nullptr, containers, workspace), blockIdx.x);
}

__global__ __launch_bounds__(64) void k_ctx_finish(uint32_t *__restrict__ status, uint8_t *__restrict__ workspace, CtxBatch b)
{
    if (threadIdx.x) return;
    ctx_finish_body(ctx_image(batch_row(b), nullptr, nullptr, nullptr, workspace), status, blockIdx.y);
}

}  // namespace

// ---- host: one path per direction, the stream length S a parameter (header dword 9); the entry points without it are S = 16384 ----
extern "C" size_t sicn_codec_ctx_max_bytes_sl(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t stream_symbols)
{
    if (!wstream_ok(stream_symbols)) return 0;
    const CtxGeom g = ctx_geom(lat_w, lat_h, lat_c, stream_symbols);
    const size_t n = (size_t)lat_w * lat_h * lat_c, ns = (size_t)g.nst[0] + g.nst[1];
    return SICN_CODEC_HEADER_BYTES + CTX_TABLE_BYTES + 4 * ns + 2 * n + 256 * ns;
}

extern "C" size_t sicn_codec_ctx_workspace_bytes_sl(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t n_images, uint32_t stream_symbols)
{
    if (!wstream_ok(stream_symbols)) return 0;
    const CtxGeom g = ctx_geom(lat_w, lat_h, lat_c, stream_symbols);
    return (size_t)n_images * ctx_ws_bytes(g.nst[0] + g.nst[1], stream_symbols);
}

extern "C" size_t sicn_codec_ctx_max_bytes(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c)
{
    return sicn_codec_ctx_max_bytes_sl(lat_w, lat_h, lat_c, WSS);
}

extern "C" size_t sicn_codec_ctx_workspace_bytes(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t n_images)
{
    return sicn_codec_ctx_workspace_bytes_sl(lat_w, lat_h, lat_c, n_images, WSS);
}

// n_images of one shape and one stream length in slots of slot_bytes: image 0's row and the strides, or SICN_EINVAL for a shape or a
// length outside the limits
static int ctx_batch(CtxBatch &b, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t img_w, uint32_t img_h, uint32_t n_images,
                     size_t slot_bytes, uint32_t S)
{
    b = CtxBatch{};
    if (n_images > 65535) return SICN_EINVAL;
    if (int rc = ctx_row_shape(b.row0, lat_w, lat_h, lat_c, img_w, img_h, S)) return rc;
    b.row0.slot_cap = ctx_slot_cap(slot_bytes);   // the caller's slots, not the layout's
    b.s_lat = (size_t)lat_w * lat_h * lat_c;
    b.s_slot = slot_bytes;
    b.s_ws = ctx_ws_bytes(b.row0.g.nst[0] + b.row0.g.nst[1], S);
    return SICN_OK;
}

extern "C" int sicn_codec_ctx_encode_batch_async_sl(const uint8_t *latents, const uint8_t *scales, uint32_t n_images, uint32_t lat_w,
                                                    uint32_t lat_h, uint32_t lat_c, uint32_t img_w, uint32_t img_h, uint8_t *out,
                                                    size_t slot_bytes, sicn_codec_status *status_dev, void *workspace,
                                                    size_t workspace_bytes, void *hip_stream, uint32_t stream_symbols)
{
    if (!latents || !scales || !out || !status_dev) return SICN_EINVAL;
    CtxBatch b;
    if (int rc = ctx_batch(b, lat_w, lat_h, lat_c, img_w, img_h, n_images, slot_bytes, stream_symbols)) return rc;
    if (n_images == 0) return SICN_OK;
    if (((uintptr_t)latents | (uintptr_t)scales) & 3) return SICN_EINVAL;   // dword gathers
    const uint32_t n = (uint32_t)b.s_lat, ns = b.row0.g.nst[0] + b.row0.g.nst[1];
    if (slot_bytes < sicn_codec_ctx_max_bytes_sl(lat_w, lat_h, lat_c, stream_symbols) || (slot_bytes & 1)) return SICN_ENOSPC;
    const size_t ws1 = b.s_ws;
    if (!workspace || workspace_bytes < ws1 * n_images) return SICN_ENOSPC;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    uint32_t *status = (uint32_t *)status_dev;
    hipLaunchKernelGGL(k_clear_stats, dim3(1, n_images), dim3(64), 0, stream, ws, stats_batch(n, n, ws1));
    HIP_TRY(hipMemset2DAsync(ws + ctx_chist_offset(), ws1, 0, NCLS * 128 * 4, n_images, stream));
    hipLaunchKernelGGL(k_stats, dim3(stats_blocks(n), n_images), dim3(256), 0, stream, latents, ws, stats_batch(n, n, ws1));
    hipLaunchKernelGGL(k_ctx_hist, dim3(b.row0.n_chunks, n_images), dim3(256), 0, stream, latents, scales, ws, b);
    hipLaunchKernelGGL(k_ctx_tables, dim3(1, n_images), dim3(1024), 0, stream, out, ws, b, 0);
    hipLaunchKernelGGL(k_ctx_enc_status, dim3(1, n_images), dim3(64), 0, stream, status, ws, b);
    hipLaunchKernelGGL(k_ctx_encode, dim3((ns + CTX_WPB - 1) / CTX_WPB, n_images), dim3(64 * CTX_WPB), 0, stream, latents, scales, ws, b);
    hipLaunchKernelGGL(k_ctx_scan, dim3(1, n_images), dim3(1024), 0, stream, out, status, ws, b, 0);
    hipLaunchKernelGGL(k_ctx_compact, dim3(ns, n_images), dim3(256), 0, stream, out, ws, b);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_codec_ctx_decode_batch_async_sl(const uint8_t *containers, size_t slot_bytes, const sicn_codec_status *valid_dev_or_null,
                                                    const uint8_t *scales, uint32_t n_images, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c,
                                                    uint8_t *latents, sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes,
                                                    void *hip_stream, uint32_t stream_symbols)
{
    if (!containers || !scales || !latents || !status_dev || (slot_bytes & 1)) return SICN_EINVAL;
    CtxBatch b;
    if (int rc = ctx_batch(b, lat_w, lat_h, lat_c, 0, 0, n_images, slot_bytes, stream_symbols)) return rc;
    if (n_images == 0) return SICN_OK;
    if (((uintptr_t)latents | (uintptr_t)scales) & 3) return SICN_EINVAL;
    const CtxGeom &g = b.row0.g;
    const uint32_t n = (uint32_t)b.s_lat;
    const size_t ws1 = b.s_ws;
    if (!workspace || workspace_bytes < ws1 * n_images) return SICN_ENOSPC;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    uint8_t *slots = const_cast<uint8_t *>(containers);   // the tables and scan kernels write containers in the encoder only
    hipLaunchKernelGGL(k_ctx_parse, dim3(1, n_images), dim3(64), 0, stream, containers, (const uint32_t *)valid_dev_or_null, ws, b);
    hipLaunchKernelGGL(k_ctx_tables, dim3(1, n_images), dim3(1024), 0, stream, slots, ws, b, 1);
    hipLaunchKernelGGL(k_ctx_scan, dim3(1, n_images), dim3(1024), 0, stream, slots, (uint32_t *)nullptr, ws, b, 1);
    // a non-anchor's class reads its neighbours' bytes whatever they hold: start from zeros so that a rejected container
    // cannot make the result depend on what the buffer held before
    HIP_TRY(hipMemsetAsync(latents, 0, (size_t)n * n_images, stream));
    hipLaunchKernelGGL(k_ctx_decode<0>, dim3((g.nst[0] + CTX_WPB_DEC - 1) / CTX_WPB_DEC, n_images), dim3(64 * CTX_WPB_DEC), 0, stream,
                       containers, scales, latents, ws, b);
    if (g.nst[1])   // (a 1 x 1 latent has no non-anchors)
        hipLaunchKernelGGL(k_ctx_decode<1>, dim3((g.nst[1] + CTX_WPB_DEC - 1) / CTX_WPB_DEC, n_images), dim3(64 * CTX_WPB_DEC), 0, stream,
                           containers, scales, latents, ws, b);
    hipLaunchKernelGGL(k_stats, dim3(stats_blocks(n), n_images), dim3(256), 0, stream, latents, ws, stats_batch(n, n, ws1));
    hipLaunchKernelGGL(k_ctx_finish, dim3(1, n_images), dim3(64), 0, stream, (uint32_t *)status_dev, ws, b);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_codec_ctx_encode_batch_async(const uint8_t *latents, const uint8_t *scales, uint32_t n_images, uint32_t lat_w,
                                                 uint32_t lat_h, uint32_t lat_c, uint32_t img_w, uint32_t img_h, uint8_t *out,
                                                 size_t slot_bytes, sicn_codec_status *status_dev, void *workspace,
                                                 size_t workspace_bytes, void *hip_stream)
{
    return sicn_codec_ctx_encode_batch_async_sl(latents, scales, n_images, lat_w, lat_h, lat_c, img_w, img_h, out, slot_bytes, status_dev,
                                                workspace, workspace_bytes, hip_stream, WSS);
}

extern "C" int sicn_codec_ctx_decode_batch_async(const uint8_t *containers, size_t slot_bytes, const sicn_codec_status *valid_dev_or_null,
                                                 const uint8_t *scales, uint32_t n_images, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c,
                                                 uint8_t *latents, sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes,
                                                 void *hip_stream)
{
    return sicn_codec_ctx_decode_batch_async_sl(containers, slot_bytes, valid_dev_or_null, scales, n_images, lat_w, lat_h, lat_c, latents,
                                                status_dev, workspace, workspace_bytes, hip_stream, WSS);
}
