/*
 * sicn_ragged_window.h — random access INSIDE an image: a pixel rectangle of each image of a ragged batch decoded from its rANS-W
 * streams without the rest of the image (library 0.12, sicn_version() >= 12).  Nothing in the container format or in the archive
 * changes: a mode-3 container is a set of independent streams, stream st holding the symbols [st * wss, st * wss + cnt) of the flat
 * [lat_h][lat_w][lat_c] latent, so a band of latent rows is a contiguous range of streams that decodes without its neighbours; and
 * the synthesis chain is local, so a rectangle of pixels needs a rectangle of the latent and no more.
 *
 * The chain.  unpack / unpack_select (sicn_ragged_archive*.h) fill a sicn_ragged_coder's slot buffer and valid array; then
 *   sicn_ragged_window_decode_async   2 launches: the streams that hold latent rows [r0, r0 + rh) of every image -> the BAND tensor
 *   sicn_ragged_cut_run               1 launch:   columns [c0, c0 + cw) of every band -> the window latents, a ragged tensor
 *   sicn_ragged_net_forward 4 .. 7    4 launches: a ragged net made for the sizes (16 cw, 16 rh) -> the windows' reconstructions
 *   sicn_ragged_cut_run               1 launch:   the rectangle out of every reconstruction -> the ROI pixels, a ragged tensor
 * whatever the number of images is.  sicn_ragged_roi_plan gives {c0, r0, cw, rh} and where the rectangle lies in the window's
 * reconstruction.  The bytes are those of the full decode of the same containers, cut to the rectangle.
 *
 * Margins.  A deconv522 layer is out[o] = sum over k of up[o + k], up[2 i + 2] = x[i].  Where its input is exact on [a + m, b - n) its
 * output is exact on [2 a + 2 m + 1, 2 b - 2 n - 2): m' = 2 m + 1, n' = 2 n + 2, from m = n = 0.  Four layers: 15 pixels on the low
 * side, 30 on the high side.  Pixels [x0, x1) need latent columns [max(0, floor((x0 - 15) / 16)), min(lat_w, ceil((x1 + 30) / 16))),
 * rows alike.  At an image's edge the window's zero padding is the image's own.
 *
 * Band.  With R = lat_w * lat_c symbols per latent row and wss the image's stream length, rows [r0, r0 + rh) lie in the streams
 * [first_stream, end_stream) = [floor(r0 R / wss), ceil((r0 + rh) R / wss)).  The band of image i holds exactly the symbols of those
 * streams, min(n, end_stream * wss) - first_stream * wss bytes at band_offset (64-bit, a multiple of 16); row r0 begins `lead` =
 * r0 R - first_stream * wss bytes into it.  No alignment is asked of the band tensor (a 4-byte aligned one takes the word stores, a
 * 16-byte aligned one the vector path of the cut).
 *
 * Verdicts.  The window decoder checks what the full decoder checks of the container's fixed part — header dwords (bit 2), frequency
 * table (bit 3), payload field (bit 4), EVERY entry of the length table (bit 5) and their sum against the payload (bit 6), a slot
 * shorter than its fixed part (bits 8 + 2) — and folds the per-stream verdicts (bit 5) over the SELECTED streams only: a damaged
 * stream outside the window is not read and not reported.  Bit 7, the Adler-32 of the whole latent, cannot be checked by a window
 * and is NEVER set here.  .bytes = the band's symbols.  An image's verdict concerns that image alone.
 *
 * One rectangle per image per call (a selection of an archive ascends strictly): two details of one photograph are two calls.
 *
 * The hyperprior configuration (sicn_ragged_ctx.h, mode 4) has its own window decoder, sicn_ragged_ctx_window.h: its y stream is
 * context-coded against a scale map that itself comes through h_s, and its windows need the halo arithmetic that header states.
 * The cut and sicn_ragged_roi_plan here serve both.
 *
 * Limits (SICN_EINVAL): those of sicn_ragged_codec_layout and sicn_ragged_crop_layout, a window with rh < 1 or r0 + rh > lat_h, a
 * rectangle that is empty or reaches outside its source.  SICN_ENODEV off gfx950 (creation and the asynchronous calls).
 */
#ifndef SICN_RAGGED_WINDOW_H
#define SICN_RAGGED_WINDOW_H

#include "sicn_ragged_codec.h"
#include "sicn_ragged_hyper.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sicn_ragged_window sicn_ragged_window;
typedef struct sicn_ragged_cut sicn_ragged_cut;

typedef struct sicn_ragged_rect {
    int32_t x0, y0, w, h;
} sicn_ragged_rect;

/* What a pixel rectangle needs of the latent, and where it lies in what layers 4 .. 7 make of that window. */
typedef struct sicn_ragged_roi {
    int32_t c0, r0, cw, rh;         /* latent columns [c0, c0 + cw), rows [r0, r0 + rh) */
    int32_t x, y;                   /* the rectangle's corner inside the window's reconstruction: x0 - (c0 << n_up_layers), y alike */
    int32_t margin_lo, margin_hi;   /* the margins the recurrences give for n_up_layers (15 and 30 for four) */
} sicn_ragged_roi;

/* Pure host, no device.  n_up_layers: the deconv522 layers between latent and pixels, 1 .. 12 (the eight-layer chain: 4).
 * SICN_EINVAL: rect empty or outside image_w x image_h, the image larger than lat << n_up_layers, a size < 1, NULL. */
int sicn_ragged_roi_plan(int n_up_layers, int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, const sicn_ragged_rect *rect,
                         sicn_ragged_roi *out);

/* Where the band of image i lies and which streams fill it. */
typedef struct sicn_ragged_window_image {
    uint64_t band_offset;           /* bytes into the band tensor, a multiple of 16 */
    uint32_t band_bytes;            /* symbols of the streams [first_stream, end_stream) */
    uint32_t first_stream, end_stream;
    uint32_t lead;                  /* latent row r0 begins at band_offset + lead */
} sicn_ragged_window_image;

/* Pure host, no device.  stream_symbols == NULL: 16384 for every image.  images_or_null: [n_images] out.  totals[2] out: bytes of the
 * band tensor, and of the workspace — the full coder's for the same images (sicn_ragged_codec_layout's totals[2]): the stage bodies
 * index their per-stream words by the stream's real number. */
int sicn_ragged_window_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                              const uint32_t *r0, const uint32_t *rh, int n_images, sicn_ragged_window_image *images_or_null,
                              uint64_t totals[2]);

/* A window decoder over an existing coder: shapes, stream lengths and slot layout are the coder's, which must outlive the window.
 * r0 / rh: [n_images] latent rows.  Uploads its tables to the current device, once.  Synchronous. */
int sicn_ragged_window_create(const sicn_ragged_coder *coder, const uint32_t *r0, const uint32_t *rh, sicn_ragged_window **out);
void sicn_ragged_window_free(sicn_ragged_window *win);
size_t sicn_ragged_window_workspace_bytes(const sicn_ragged_window *win);

/* The contract of sicn_ragged_coder_decode_async: enqueue only, no allocation, no host synchronisation, capturable into a hipGraph,
 * one call in flight per workspace; SICN_EINVAL (NULL, a workspace that is not 16-byte aligned) and SICN_ENOSPC (a workspace smaller
 * than sicn_ragged_window_workspace_bytes) before any launch.  containers / valid_dev_or_null: the coder's slot buffer and valid
 * array.  band: the band tensor of sicn_ragged_window_layout; nothing outside the bands is written.  status_dev[n_images]: the
 * verdicts described above.  TWO launches whatever n_images is. */
int sicn_ragged_window_decode_async(const sicn_ragged_window *win, const uint8_t *containers, const sicn_codec_status *valid_dev_or_null,
                                    uint8_t *band, sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes,
                                    void *hip_stream);

/* The cut: destination image i = the [h][w][channels] rectangle at (x0, y0) of source image i; the destination is a ragged tensor,
 * back to back.  Source images lie back to back, or at src_offset[i] bytes (64-bit; how the latent cut reads a band at
 * band_offset + lead, with src_w = lat_w, src_h = the rows the band holds from r0 on).  One launch; a work item is
 * SICN_RAGGED_CROP_ROWS destination rows.  16-byte vectors where both row pitches, the rectangle's byte offset, both image offsets
 * and both base pointers allow; byte by byte otherwise.
 * sicn_ragged_cut_layout, pure host: out[] = { byte offset of source image `image`, of the destination image, bytes of the source
 * tensor (with src_offset: the furthest byte any source image reaches), bytes of the destination tensor }.
 * SICN_EINVAL: the limits of sicn_ragged_crop_layout, a rectangle that is empty or outside its source. */
int sicn_ragged_cut_layout(const int32_t *src_w, const int32_t *src_h, const sicn_ragged_rect *rects, int channels,
                           const uint64_t *src_offset_or_null, int n_images, int image, int64_t out[4]);
int sicn_ragged_cut_create(const int32_t *src_w, const int32_t *src_h, const sicn_ragged_rect *rects, int channels,
                           const uint64_t *src_offset_or_null, int n_images, sicn_ragged_cut **out);
void sicn_ragged_cut_free(sicn_ragged_cut *cut);
/* Enqueue only, capturable. */
int sicn_ragged_cut_run(const sicn_ragged_cut *cut, const uint8_t *src, uint8_t *dst, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_WINDOW_H */
