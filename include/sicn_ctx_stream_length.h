/*
 * sicn_ctx_stream_length.h — the stream length of the rANS-WC coder (container mode 4 of sicn_codec.h) as an ENCODER PARAMETER
 * (library 0.14, sicn_version() >= 14), through the uniform coder, the ragged coder (sicn_ragged_ctx.h) and the window decoder's
 * plan (sicn_ragged_ctx_window.h).  Mode 4 stays mode 4: header dword 9 is the stream length S, a power of two in 1024 .. 16384;
 * each checkerboard set is cut into streams of S symbols; the class rule and the 16 tables do not depend on S; a container of
 * S = 16384 is byte for byte what the entry points without a length write.  All of it is new symbols: no prototype and no struct
 * of the headers named above changes, and their entry points are the S = 16384 case of the same host paths.
 */
#ifndef SICN_CTX_STREAM_LENGTH_H
#define SICN_CTX_STREAM_LENGTH_H

#include "sicn_ragged_ctx_window.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Mode 4 with the STREAM LENGTH as an encoder parameter (library 0.14, sicn_version() >= 14): stream_symbols = a power of two,
 * 1024 .. 16384, written to header dword 9.  The four mode-4 entry points of sicn_codec.h are these at 16384, byte for
 * byte.  The size functions return 0 for a length that is not admissible, the asynchronous calls SICN_EINVAL before anything is enqueued.  Size
 * slots and workspace with the same length the coder calls get.  Every stream ends with 260 bytes of flush (64 final states and a
 * length entry), so shorter streams cost bytes; they buy a shorter serial chain per wave (stream_symbols / 256 blocks) and a finer
 * selection of rows in the window decoder (sicn_ragged_ctx_window.h). */
size_t sicn_codec_ctx_max_bytes_sl(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t stream_symbols);
size_t sicn_codec_ctx_workspace_bytes_sl(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t n_images, uint32_t stream_symbols);
int sicn_codec_ctx_encode_batch_async_sl(const uint8_t *latents, const uint8_t *scales, uint32_t n_images, uint32_t lat_w,
                                         uint32_t lat_h, uint32_t lat_c, uint32_t image_width, uint32_t image_height, uint8_t *out,
                                         size_t slot_bytes, sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes,
                                         void *hip_stream, uint32_t stream_symbols);
int sicn_codec_ctx_decode_batch_async_sl(const uint8_t *containers, size_t slot_bytes, const sicn_codec_status *valid_dev_or_null,
                                         const uint8_t *scales, uint32_t n_images, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c,
                                         uint8_t *latents, sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes,
                                         void *hip_stream, uint32_t stream_symbols);

/* sicn_ragged_ctx_layout / sicn_ragged_ctx_coder_create (sicn_ragged_ctx.h) with a STREAM LENGTH PER IMAGE:
 * stream_symbols_or_null[n_images], each a power of two in 1024 .. 16384 (header dword 9 of image i's container); NULL = 16384 for every image, which is those two calls.
 * slot_bytes = sicn_codec_ctx_max_bytes_sl of the image's length rounded up to 16, the workspace block is sized by it, and
 * anchor_streams / nonanchor_streams count streams of that length.  A length that is not admissible, or an image whose streams'
 * scratch would pass 2^32 bytes (sicn_codec.h, mode 4), is SICN_EINVAL before anything is made.  The lengths live in the coder
 * object: sicn_ragged_ctx_encode_async writes them, sicn_ragged_ctx_decode_async and a window decoder made from the coder
 * expect them (a container of another length: bit 2, for that image alone). */
int sicn_ragged_ctx_layout_sl(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                              int n_images, sicn_ragged_ctx_image *images_or_null, uint64_t totals[3]);
int sicn_ragged_ctx_coder_create_sl(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                                    const uint32_t *image_w_or_null, const uint32_t *image_h_or_null, int n_images,
                                    sicn_ragged_ctx_coder **out);

/* sicn_ragged_ctx_window_layout (sicn_ragged_ctx_window.h) with a stream length per image: stream_symbols_or_null[n_images] as in
 * sicn_ragged_ctx_layout_sl, NULL = 16384 for every image; the plan of that header's comment with the image's S.  A window decoder takes the lengths from its coder (sicn_ragged_ctx_coder_create_sl). */
int sicn_ragged_ctx_window_layout_sl(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                                     const uint32_t *r0, const uint32_t *rh, int n_images,
                                     sicn_ragged_ctx_window_image *images_or_null, uint64_t totals[2]);

#ifdef __cplusplus
}
#endif
#endif /* SICN_CTX_STREAM_LENGTH_H */
