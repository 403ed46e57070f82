/*
 * sicn_ragged_ctx_window.h — random access INSIDE an image of the hyperprior configuration: a window of latent rows of each image of
 * a ragged batch decoded from its rANS-WC streams (container mode 4, sicn_ragged_ctx.h) without the other streams of the image
 * (library 0.13, sicn_version() >= 13).  Nothing in the container format or in the archive changes: a mode-4 container is two sets
 * of independent streams of S symbols (header dword 9, the image's stream length: 16384 unless the encoder chose less, library
 * 0.14), anchors ((x + y) even) then non-anchors; inside a set the pixels lie in raster order over
 * ROW PAIRS — pair p holds the set's pixels of rows 2 p and 2 p + 1, R = lat_w * lat_c symbols of either set — so a band of latent
 * rows is a contiguous range of streams in each set.  The only coupling between streams is the class rule: the class of a non-anchor
 * symbol reads its four anchor neighbours, and one symbol decoded with a wrong class corrupts its lane's rANS state for the rest of
 * its stream.  So EVERY symbol of a selected non-anchor stream needs all its anchor neighbours decoded, not only the symbols of the
 * rows asked for: that is the halo below.
 *
 * Plan, for one image W = lat_w, H = lat_h, C = lat_c (C % 4 == 0), nsym[2] / nst[2] the symbols / streams of the two sets, S its
 * stream length, rows wanted [r0, r1 = r0 + rh):
 *   non-anchor streams   lo = (r0 >> 1) R, hi = min(nsym[1], ((r1 + 1) >> 1) R).  hi > lo: [N0, N1) = [lo / S, ceil(hi / S)),
 *                        which touch the row pairs [P0, P1) = [N0 S / R, ceil(min(nsym[1], N1 S) / R)).  Else none.
 *   anchor rows          the wanted rows and every neighbour of every non-anchor the selected streams hold:
 *                        [A0, A1) = [max(0, min(r0, 2 P0 - 1)), min(H, max(r1, 2 P1 + 1))); without non-anchor streams [r0, r1).
 *   anchor streams       [M0, M1) = [(A0 >> 1) R / S, ceil(min(nsym[0], ((A1 + 1) >> 1) R) / S)), touching the pairs [Q0, Q1)
 *                        by the formula of P.
 *   band                 whole latent rows [band_row0, band_row0 + band_rows) = [2 min(P0, Q0), min(H, 2 max(P1, Q1))) at full
 *                        width (without non-anchor streams: Q alone), band_bytes = band_rows W C.
 * Whole row pairs always; a tighter plan (half pairs for an odd r0) is not made.  Streams shorter than a row pair (S < R) select
 * rows more finely: the band of a window can only shrink as S does.
 *
 * Band.  Image i's band lies at band_offset (64-bit, a multiple of 16) of the band tensor, the images back to back; wanted row r0
 * begins (r0 - band_row0) W C bytes into it.  After a decode the band holds, at every position of its rows, the symbol of the
 * latent where a selected stream holds that position and ZERO elsewhere (the decoder zeroes the band tensor first).  The band
 * tensor must be 4-byte aligned (the class rule gathers dwords).
 *
 * Verdicts.  The window decoder checks what the full decoder checks of the container's fixed part — header dwords (bit 2), class
 * tables (bit 3), payload field (bit 4), EVERY entry of the length table (bit 5) and their sum against the payload (bit 6), a slot
 * shorter than its fixed part (bits 8 + 2) — and the SELECTED streams (bit 5): a damaged stream outside the window is neither read
 * nor reported.  Bit 7, the Adler-32 of the whole latent, cannot be checked by a window and is NEVER set here.  .bytes = the symbols
 * the selected streams hold.  An image's verdict concerns that image alone.
 *
 * The scale maps are the FULL ones: the hyper-synthesis ends at latent resolution and is run in full; a windowed h_s is out of scope.
 *
 * Limits (SICN_EINVAL): those of sicn_ragged_ctx_layout, a window with rh < 1 or r0 + rh > lat_h, a null pointer.  SICN_ENODEV off
 * gfx950 (creation and the asynchronous call).
 */
#ifndef SICN_RAGGED_CTX_WINDOW_H
#define SICN_RAGGED_CTX_WINDOW_H

#include "sicn_ragged_ctx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sicn_ragged_ctx_window sicn_ragged_ctx_window;

/* Where the band of image i lies and which streams fill it. */
typedef struct sicn_ragged_ctx_window_image {
    uint64_t band_offset;               /* bytes into the band tensor, a multiple of 16 */
    uint32_t band_bytes;                /* band_rows * lat_w * lat_c */
    uint32_t band_row0, band_rows;      /* the whole latent rows the band holds */
    uint32_t first_stream[2], end_stream[2];   /* per set (anchors, non-anchors), in the set's own numbering */
    uint32_t symbols;                   /* what the selected streams hold */
} sicn_ragged_ctx_window_image;

/* Pure host, no device.  r0 / rh: [n_images] latent rows.  images_or_null: [n_images] out.  totals[2] out: bytes of the band tensor,
 * and of the workspace — the full ctx coder's for the same images (sicn_ragged_ctx_layout's totals[2]): the stages index their
 * per-stream words by the stream's real number. */
int sicn_ragged_ctx_window_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *r0, const uint32_t *rh,
                                  int n_images, sicn_ragged_ctx_window_image *images_or_null, uint64_t totals[2]);

/* A window decoder over an existing coder: shapes and slot layout are the coder's, which must outlive the window.  Uploads its
 * tables to the current device, once.  Synchronous. */
int sicn_ragged_ctx_window_create(const sicn_ragged_ctx_coder *coder, const uint32_t *r0, const uint32_t *rh, sicn_ragged_ctx_window **out);
void sicn_ragged_ctx_window_free(sicn_ragged_ctx_window *win);
size_t sicn_ragged_ctx_window_workspace_bytes(const sicn_ragged_ctx_window *win);

/* The contract of sicn_ragged_ctx_decode_async: enqueue only, no allocation, no host synchronisation, capturable into a hipGraph, one
 * call in flight per workspace.  containers / valid_dev_or_null: the coder's slot buffer and valid array.  scales: the ragged tensor
 * of FULL scale maps in the coder's latent layout.  band: the band tensor of sicn_ragged_ctx_window_layout; nothing outside it is
 * written.  status_dev[n_images]: the verdicts described above.  SEVEN enqueued operations whatever n_images is (SIX when no image
 * selects a non-anchor stream): a memset of the band tensor — first, so that a rejected container cannot make the result depend on
 * what the buffer held — parse, tables, scan, the anchor streams, the non-anchor streams, the verdicts.
 * SICN_EINVAL (NULL, scales or band not 4-byte aligned, containers not 2-byte aligned, a workspace not 16-byte aligned) and
 * SICN_ENOSPC (a workspace smaller than sicn_ragged_ctx_window_workspace_bytes) before any launch. */
int sicn_ragged_ctx_window_decode_async(const sicn_ragged_ctx_window *win, const uint8_t *containers,
                                        const sicn_codec_status *valid_dev_or_null, const uint8_t *scales, uint8_t *band,
                                        sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_CTX_WINDOW_H */
