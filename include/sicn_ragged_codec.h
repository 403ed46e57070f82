/*
 * sicn_ragged_codec.h — the rANS-W coder (container mode 3 of sicn_codec.h) over n latents of n DIFFERENT shapes: n SICL containers
 * from THREE kernel launches for the whole batch, n latents back from TWO, whatever n is (library 0.7, sicn_version() >= 7).  It
 * is the coder of a ragged batch (sicn_ragged.h): the ragged latent tensor, boundary 3 of the ragged net, goes in as it lies.
 *
 * Bytes.  Container i is byte-identical to what sicn_codec_encode_batch_async_sl writes for image i alone with the same stream
 * length, and to the oracle's (oracle/sicn_codec_oracle.c); a container written here decodes with sicn_codec_decode and the other
 * way round.  The container format is unchanged and there is no new mode.  The stream length is PER IMAGE, never per call: the
 * bitstream of an image does not depend on what was coded beside it (codec.auto_stream_symbols of that image's latent is the
 * Python default).
 *
 * Data model.  Latents: the images' [lat_h][lat_w][lat_c] uint8 arrays back to back, no padding (values < 128), image i at
 * latent_offset = sum over j < i of n_symbols(j) — with equal shapes the [n][h][w][c] batch of sicn_codec.h.  Containers: one SLOT
 * per image in one buffer, at slot_offset, of slot_bytes = sicn_codec_max_bytes_sl(n_symbols, stream_symbols) rounded up to a
 * multiple of 16; the bytes of a slot behind its container are never written.  Offsets are 64-bit: the latent tensor and the slot
 * buffer may exceed 2 GiB.  No alignment is asked of the latents or the slot buffer (16-byte aligned buffers take the vector paths);
 * the workspace must be 16-byte aligned.
 *
 * Kernels.  The stages of the uniform coder (csrc/k_codec_body.hpp) on a FLAT grid over the work items of all images — statistics
 * rows, then streams — each workgroup finding its image through tables the coder object uploads once.  Only the SELF-SCANNING
 * form of the coder exists here (every stream sums the length table up to itself; no scan kernel): an image of more than 2048
 * streams is SICN_EINVAL — the ragged coder has no other form to fall back on.  That is 2 M symbols at 1024-symbol streams and
 * 32 M symbols (a 6688 x 6688 image's latent of 192 channels) at 16384.
 *
 * Limits (SICN_EINVAL): n_images < 1, a latent dimension < 1, stream_symbols[i] not a power of two in 1024 .. 16384, an image of
 * more than 2048 streams, >= 2^31 - 1 streams in all.  SICN_ENODEV off gfx950 (creation and the two asynchronous calls).
 */
#ifndef SICN_RAGGED_CODEC_H
#define SICN_RAGGED_CODEC_H

#include "sicn_codec.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sicn_ragged_coder sicn_ragged_coder;

/* Where image i lies and how it is cut. */
typedef struct sicn_ragged_codec_image {
    uint64_t latent_offset;    /* bytes into the ragged latent tensor */
    uint64_t slot_offset;      /* bytes into the slot buffer, a multiple of 16 */
    uint64_t workspace_offset; /* bytes into the workspace: the image's block, laid out as the uniform coder's */
    uint32_t slot_bytes;       /* capacity of the slot */
    uint32_t n_symbols, n_streams, stream_symbols;
} sicn_ragged_codec_image;

/* Pure host, no device.  stream_symbols == NULL: 16384 for every image.  images_or_null: [n_images] out.
 * totals[3] out: bytes of the latent tensor, of the slot buffer, of the workspace. */
int sicn_ragged_codec_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                             int n_images, sicn_ragged_codec_image *images_or_null, uint64_t totals[3]);

/* image_w / image_h: header fields only (NULL: 0).  Uploads the lookup tables to the current device, once.  Synchronous. */
int sicn_ragged_coder_create(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                             const uint32_t *image_w_or_null, const uint32_t *image_h_or_null, int n_images,
                             sicn_ragged_coder **out);
void sicn_ragged_coder_free(sicn_ragged_coder *coder);
size_t sicn_ragged_coder_workspace_bytes(const sicn_ragged_coder *coder);

/* The contract of sicn_codec_encode_batch_async / sicn_codec_decode_batch_async: enqueue only, no allocation, no host
 * synchronisation, capturable into a hipGraph, one call in flight per workspace; results in DEVICE memory, status_dev[n_images],
 * with the error bits sicn_codec.h documents (encode: bit 0 a symbol >= 128, bit 1 no valid frequency table, .bytes = container
 * size; decode: bits 2-6 malformed container, bit 7 checksum mismatch, bit 8 slot shorter than its fixed part, .bytes = symbols
 * decoded).  An image's verdict concerns that image alone: the others are coded as if it were not there.
 * valid_dev_or_null[i].bytes bounds what the decoder reads of slot i (e.g. the encoder's status array); NULL = the whole slot.
 * The decoder takes every shape and stream length from the coder object; a container whose header disagrees is an error (bit 2).
 * SICN_ENOSPC, nothing enqueued, when the workspace is smaller than sicn_ragged_coder_workspace_bytes. */
int sicn_ragged_coder_encode_async(const sicn_ragged_coder *coder, const uint8_t *latents, uint8_t *containers,
                                   sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes, void *hip_stream);
int sicn_ragged_coder_decode_async(const sicn_ragged_coder *coder, const uint8_t *containers,
                                   const sicn_codec_status *valid_dev_or_null, uint8_t *latents, sicn_codec_status *status_dev,
                                   void *workspace, size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_CODEC_H */
