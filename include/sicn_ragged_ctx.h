/*
 * sicn_ragged_ctx.h — the rANS-WC coder (container mode 4 of sicn_codec.h, the conditional coder of the hyperprior configuration)
 * over n latents of n DIFFERENT shapes, each with its scale map: n SICL mode-4 containers from SIX launches for the whole batch,
 * n latents back from EIGHT (one of them a memset), whatever n is (library 0.9, sicn_version() >= 9).  It is the y coder of a ragged
 * hyperprior batch (sicn_ragged_hyper.h): the ragged latent tensor and the cropped scale maps go in as they lie.
 *
 * Bytes.  Container i is byte-identical to what sicn_codec_ctx_encode_batch_async writes for image i alone, and to the oracle's
 * (oracle/sicn_hyper_oracle.c); a container written here decodes with sicn_codec_ctx_decode_batch_async and the other way round.
 * The container format is unchanged and there is no new mode.  Streams are 16384 symbols long here; sicn_ctx_stream_length.h
 * (library 0.14) makes a coder with a length per image, which these encode / decode calls then write and expect.
 *
 * Data model.  Latents and scales: two ragged tensors of ONE layout, the images' [lat_h][lat_w][lat_c] uint8 arrays back to back,
 * no padding (values < 128), image i at latent_offset = sum over j < i of n_symbols(j).  lat_c is common to the batch and a multiple
 * of 4, so every image starts at a multiple of 4 bytes: the class rule gathers dwords, and both tensors must be 4-byte aligned.
 * Containers: one SLOT per image in one buffer, at slot_offset, of slot_bytes = sicn_codec_ctx_max_bytes(lat_w, lat_h, lat_c)
 * rounded up to a multiple of 16; the bytes of a slot behind its container are never written.  Workspace: one block per image, at
 * workspace_offset, laid out as the uniform coder's; the workspace must be 16-byte aligned.  Offsets are 64-bit: the tensors, the
 * slot buffer and the workspace may exceed 4 GiB.
 *
 * Kernels.  The stages of the uniform coder (csrc/k_ctx_body.hpp: functions of one image) on FLAT grids over the work
 * items of all images — chunks of dwords for the statistics, groups of streams for the coders, single streams for the compaction,
 * whole images for tables, parse, scan and verdict — each workgroup finding its image through tables the coder object uploads once.
 * An image has as many streams as its shape gives (no per-image limit, as in the uniform coder).
 *
 * Limits (SICN_EINVAL): n_images < 1, a latent dimension < 1, lat_c not a multiple of 4, an image of more than 0x7F000000 symbols
 * (the uniform coder's limit), >= 2^31 - 1 streams in all, a null pointer, latents or scales not 4-byte aligned, the decoder's
 * containers not 2-byte aligned (it reads the streams as 16-bit words; slot offsets are even), a workspace not 16-byte aligned.
 * SICN_ENODEV off gfx950 (creation and the two asynchronous calls).
 */
#ifndef SICN_RAGGED_CTX_H
#define SICN_RAGGED_CTX_H

#include "sicn_codec.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sicn_ragged_ctx_coder sicn_ragged_ctx_coder;

/* Where image i lies and how it is cut. */
typedef struct sicn_ragged_ctx_image {
    uint64_t latent_offset;    /* bytes into the ragged latent tensor and into the ragged scale tensor, a multiple of 4 */
    uint64_t slot_offset;      /* bytes into the slot buffer, a multiple of 16 */
    uint64_t workspace_offset; /* bytes into the workspace: the image's block, laid out as the uniform coder's */
    uint64_t slot_bytes;       /* capacity of the slot */
    uint32_t n_symbols;
    uint32_t anchor_streams, nonanchor_streams; /* streams of the two checkerboard sets, in container order */
} sicn_ragged_ctx_image;

/* Pure host, no device.  images_or_null: [n_images] out.
 * totals[3] out: bytes of the latent tensor (and of the scale tensor), of the slot buffer, of the workspace. */
int sicn_ragged_ctx_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, int n_images,
                           sicn_ragged_ctx_image *images_or_null, uint64_t totals[3]);

/* image_w / image_h: header fields only (NULL: 0).  Uploads the lookup tables to the current device, once.  Synchronous. */
int sicn_ragged_ctx_coder_create(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *image_w_or_null,
                                 const uint32_t *image_h_or_null, int n_images, sicn_ragged_ctx_coder **out);
void sicn_ragged_ctx_coder_free(sicn_ragged_ctx_coder *coder);
size_t sicn_ragged_ctx_coder_workspace_bytes(const sicn_ragged_ctx_coder *coder);

/* The contract of sicn_codec_ctx_encode_batch_async / sicn_codec_ctx_decode_batch_async: enqueue only, no allocation, no host
 * synchronisation, capturable into a hipGraph, one call in flight per workspace; results in DEVICE memory, status_dev[n_images],
 * with the error bits sicn_codec.h documents (encode: bit 0 a symbol or a scale >= 128, bit 1 no valid frequency table, .bytes =
 * container size; decode: bits 2-6 malformed container, bit 7 checksum mismatch, bit 8 slot shorter than its fixed part, .bytes =
 * symbols decoded).  An image's verdict concerns that image alone: the others are coded as if it were not there.
 * valid_dev_or_null[i].bytes bounds what the decoder reads of slot i (e.g. the encoder's status array); NULL = the whole slot.
 * The decoder takes every shape from the coder object; a container whose header disagrees is an error (bit 2).  It zeroes the
 * latent tensor first (one memset), so what a rejected container leaves behind does not depend on what the buffer held.
 * SICN_ENOSPC, nothing enqueued, when the workspace is smaller than sicn_ragged_ctx_coder_workspace_bytes.  SICN_EINVAL likewise
 * enqueues nothing.  SICN_ENODEV from the decoder's memset (its first node) enqueues nothing either; SICN_ENODEV after the launches
 * (hipGetLastError) means a launch was refused: what is on the stream is then unspecified and the outputs must not be used. */
int sicn_ragged_ctx_encode_async(const sicn_ragged_ctx_coder *coder, const uint8_t *latents, const uint8_t *scales,
                                 uint8_t *containers, sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes,
                                 void *hip_stream);
int sicn_ragged_ctx_decode_async(const sicn_ragged_ctx_coder *coder, const uint8_t *containers,
                                 const sicn_codec_status *valid_dev_or_null, const uint8_t *scales, uint8_t *latents,
                                 sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_CTX_H */
