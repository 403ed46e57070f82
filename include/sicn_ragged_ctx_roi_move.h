/*
 * sicn_ragged_ctx_roi_move.h — the moving ROI decode of sicn_ragged_roi_move.h for the HYPERPRIOR configuration: rectangles of fixed
 * size whose positions are read from device memory on every call, decoded from the rANS-WC streams (container mode 4) of a ragged
 * batch.  Nothing in the container format, in the archive, in any existing symbol or struct or in any existing kernel changes, and
 * sicn_version() stays 17: THE PRESENCE OF THE SYMBOLS BELOW IS THE MARKER of this extension.
 *
 * Why.  sicn_ragged_ctx_window_create bakes one set of latent rows into its tables, the two cuts and the window's ragged net bake
 * the rectangles into theirs, and every decode of that chain runs again what does not depend on the rectangle at all: the parse,
 * tables and scan stages of the container's fixed part (and, above this header, the z coder and the hyper-synthesis).  Here the
 * objects are made ONCE for a list of SLOTS, the fixed part is read ONCE per set of containers (prepare), and a move costs its own
 * launches alone (decode).
 *
 * Slots.  sicn_ragged_roi_slot { image, w, h } with the semantics of sicn_ragged_roi_move.h: sizes are fixed, several slots may name
 * one image, in any order.  What moves is the position (x0, y0), an int32 pair in device memory, read when the kernels run.
 *
 * Pixel axes.  Exactly sicn_ragged_roi_move.h's, with n_up_layers = SICN_ROI_MOVE_UP_LAYERS: cw_cap and rh_cap are
 * sicn_ragged_roi_move_capacity's; the clamp, the flag SICN_ROI_MOVE_CLAMPED, c0, r0 and the corner (x, y) are
 * sicn_ragged_roi_move_place's.  The placed window is the latent rows [r0, r0 + rh_cap), r0 in [0, lat_h - rh_cap], and the
 * columns [c0, c0 + cw_cap).
 *
 * Streams and band.  For a placed r0 the plan of sicn_ragged_ctx_window.h for the rows [r0, r0 + rh_cap) of the slot's image, at the
 * image's stream length S, gives the anchor streams [M0, M1), the non-anchor streams [N0, N1) and the band rows [B0, B1).  The
 * device evaluates that plan itself, by the very function the host entry points call (csrc/ctx_window_host.hpp plan_of_sl through
 * csrc/ctx_roi_move_host.hpp).
 *
 * Capacity (pure host, sicn_ragged_ctx_roi_move_capacity).  max_streams[0] = max (M1 - M0), max_streams[1] = max (N1 - N0) and
 * band_rows_cap = max (B1 - B0) over ALL admissible r0, found by enumeration (O(lat_h)): exact maxima, each attained at some
 * position.  They vary with the position (a 37 x 37 x 192 latent at S = 1024 and rh_cap = 5: 25 .. 50 anchor streams, 18 .. 22
 * non-anchor streams, 9 .. 18 band rows), so most calls leave surplus work items, which return before they read anything else.
 * A 1 x 1 latent has no non-anchor stream: max_streams[1] = 0.
 *
 * Layout (pure host, sicn_ragged_ctx_roi_move_layout).  Per slot, in slot order, back to back:
 *   a band of band_rows_cap * lat_w * lat_c bytes at band_offset (64-bit, a multiple of 16): the placed band's row B0 is its first;
 *   its window latent [rh_cap][cw_cap][lat_c], its reconstruction [16 rh_cap][16 cw_cap][3] and its pixels [h][w][3] — the layouts
 *     of a ragged net made for the sizes (16 cw_cap, 16 rh_cap), as in sicn_ragged_roi_move.h;
 *   per set a fixed range of items[set] = ceil(max_streams[set] / SICN_CTX_ROI_MOVE_STREAMS_PER_ITEM) work items of that set's
 *     decode grid, from first_item[set].
 * Workspace: the FULL ctx coder's for the coder's images (sicn_ragged_ctx_layout's totals[2]) + 64 bytes per slot, slot k's at
 * meta_offset = that total + 64 k: its own `meta` block.  The images' blocks hold the tables and stream offsets, which a decode only
 * reads; everything a decode writes to the workspace is the slot's block: two slots of one image share nothing writable.
 *
 * Two calls, because two things change at different rates.
 *   sicn_ragged_ctx_roi_move_prepare_async   once per set of containers.  THREE launches: the parse, tables (decoder form) and
 *     scan (decoder form) stages of the coder over the DISTINCT images the slots name, into those images' workspace blocks.  The
 *     containers of other images are not read.
 *   sicn_ragged_ctx_roi_move_decode_async    once per move.  Reads what the last prepare ON THE SAME WORKSPACE left there: the
 *     containers (and valid array) must be THE SAME BYTES that prepare read.  SIX enqueued operations whatever n_slots is (FIVE
 *     when no slot has non-anchor capacity), linear — a captured graph of it has no parallel branches:
 *       1. the placement, one thread per slot: clamp and place, the plan, the slot's row (first[2], end[2], symbols, lat_bias =
 *          band_offset - B0 lat_w lat_c), the two cuts' rows (the latent cut reads at band_offset + (r0 - B0) lat_w lat_c + c0
 *          lat_c), the flag word, and the RESET of the slot's meta block from its image's meta[0..3] as prepare left them;
 *       2. a memset of the whole band tensor (a fixed size): the class rule reads neighbours whatever they hold;
 *       3. the anchor streams, 4. the non-anchor streams: flat grids, fixed per set; a work item whose first stream is >= end[set]
 *          returns before it loads the class tables; otherwise the coder's decode stage runs unchanged with the stream's real index,
 *          the latent biased into the slot's band and the error word the slot's own;
 *       5. one verdict per SLOT;
 *       6. the latent cut: band -> window latents.
 *   sicn_ragged_net_forward 4 .. 7 of a ragged net made for the sizes (16 cw_cap, 16 rh_cap), then
 *   sicn_ragged_ctx_roi_move_cut_async       ONE launch: the rectangles out of the reconstructions -> the ROI pixels.
 *
 * After a decode the slot's band holds, at every position of the rows [B0, B1), the symbol of the latent where a selected stream
 * holds that position and ZERO elsewhere, as in sicn_ragged_ctx_window.h; the rows [r0, r0 + rh_cap) are complete.
 *
 * Verdicts.  status_dev[n_slots]: those of sicn_ragged_ctx_window_decode_async for the slot's IMAGE — the container's fixed part as
 * prepare found it: header (bit 2), class tables (bit 3), payload field (bit 4), every entry of the length table (bit 5), their sum
 * (bit 6), a slot shorter than its fixed part (bits 8 + 2) — and for the streams the slot selected IN THIS CALL (bit 5).  Bit 7 is
 * never set.  .bytes = the symbols of the selected streams.  A damaged stream that a slot moves off is no longer reported, and a
 * slot's verdict concerns that slot alone.
 *
 * One call in flight per object (the placement writes the object's own device tables) and per workspace.
 *
 * Limits (SICN_EINVAL): n_slots < 1, an image index out of range, those of sicn_ragged_roi_move_layout (w or h < 1 or larger than
 * the image, an image without a size or larger than 16 x its latent, a reconstruction of 2^31 bytes, 2^31 - 1 work items) and of
 * sicn_ragged_ctx_layout (lat_c % 4, the stream length, the symbols of one image).  SICN_ENODEV off gfx950 (creation and the
 * asynchronous calls).
 */
#ifndef SICN_RAGGED_CTX_ROI_MOVE_H
#define SICN_RAGGED_CTX_ROI_MOVE_H

#include "sicn_ragged_ctx_window.h"
#include "sicn_ragged_roi_move.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SICN_CTX_ROI_MOVE_STREAMS_PER_ITEM 8    /* streams of one set that one work item of a decode grid takes */

typedef struct sicn_ragged_ctx_roi_move sicn_ragged_ctx_roi_move;

/* What a position means for a slot: the pixel axes, and the plan of the placed rows. */
typedef struct sicn_ragged_ctx_roi_placed {
    sicn_ragged_roi_placed px;                  /* sicn_ragged_roi_move_place's */
    uint32_t first_stream[2], end_stream[2];    /* per set (anchors, non-anchors), in the set's own numbering */
    uint32_t band_row0, band_rows;              /* the whole latent rows the selected streams fill */
    uint32_t symbols;                           /* what the selected streams hold */
    uint32_t pad;
    uint64_t lat_bias;                          /* band_offset - band_row0 lat_w lat_c, modulo 2^64 */
    uint64_t cut_offset;                        /* where the latent cut reads: the window's first byte in the band tensor */
} sicn_ragged_ctx_roi_placed;

/* Where a slot lies in the tensors of the chain. */
typedef struct sicn_ragged_ctx_roi_move_slot {
    uint64_t band_offset;                       /* a multiple of 16; the band's capacity is band_rows_cap * lat_w * lat_c bytes */
    uint64_t latent_offset, recon_offset, roi_offset;
    uint64_t meta_offset;                       /* the slot's 64 bytes of the workspace */
    uint32_t cw_cap, rh_cap, band_rows_cap;
    uint32_t max_streams[2], first_item[2], items[2];
    uint32_t pad;
} sicn_ragged_ctx_roi_move_slot;

/* Pure host, no device.  The capacities of a window of rh_cap rows that moves over a [lat_h][lat_w][lat_c] latent cut into streams
 * of stream_symbols: cap[3] out = { max_streams[0], max_streams[1], band_rows_cap }.  SICN_EINVAL: the limits of
 * sicn_ragged_ctx_window_layout, rh_cap < 1 or > lat_h, NULL. */
int sicn_ragged_ctx_roi_move_capacity(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t stream_symbols, uint32_t rh_cap,
                                      uint32_t cap[3]);
/* Pure host, no device.  Any int32 position is admissible: it is clamped.  band_offset: the slot's (0 for the plan alone). */
int sicn_ragged_ctx_roi_move_place(int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, uint32_t lat_c, uint32_t stream_symbols,
                                   int32_t w, int32_t h, int32_t x0, int32_t y0, uint64_t band_offset, sicn_ragged_ctx_roi_placed *out);

/* Pure host, no device.  The first five arguments as in sicn_ragged_ctx_layout_sl; image_w / image_h: [n_images] pixels.
 * slots_out_or_null: [n_slots].  totals[7] out: bytes of the band tensor, of the window latents, of the reconstructions, of the ROI
 * pixels and of the workspace, and the work items of the anchor and of the non-anchor decode grid. */
int sicn_ragged_ctx_roi_move_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                                    const uint32_t *image_w, const uint32_t *image_h, int n_images, const sicn_ragged_roi_slot *slots,
                                    int n_slots, sicn_ragged_ctx_roi_move_slot *slots_out_or_null, uint64_t totals[7]);

/* Over an existing ctx coder made WITH image sizes, which must outlive the object.  Allocates and uploads its tables on the current
 * device, once; the rows the placement writes start as the placement of (0, 0).  Synchronous. */
int sicn_ragged_ctx_roi_move_create(const sicn_ragged_ctx_coder *coder, const sicn_ragged_roi_slot *slots, int n_slots,
                                    sicn_ragged_ctx_roi_move **out);
void sicn_ragged_ctx_roi_move_free(sicn_ragged_ctx_roi_move *mv);
size_t sicn_ragged_ctx_roi_move_workspace_bytes(const sicn_ragged_ctx_roi_move *mv);

/* The family's contract, all three: enqueue only, no allocation, no host synchronisation, capturable into a hipGraph; SICN_EINVAL
 * (NULL, scales or band not 4-byte aligned, containers not 2-byte aligned, a workspace not 16-byte aligned, positions not 4-byte
 * aligned) and SICN_ENOSPC (a workspace smaller than sicn_ragged_ctx_roi_move_workspace_bytes) before any launch.
 * containers / valid_dev_or_null: the coder's slot buffer and valid array (indexed by IMAGE).  THREE launches. */
int sicn_ragged_ctx_roi_move_prepare_async(const sicn_ragged_ctx_roi_move *mv, const uint8_t *containers,
                                           const sicn_codec_status *valid_dev_or_null, void *workspace, size_t workspace_bytes,
                                           void *hip_stream);
/* xy_dev: [n_slots] pairs { x0, y0 } in device memory, read when the kernels run.  containers: THE SAME BYTES the last prepare on
 * this workspace read.  scales: the ragged tensor of FULL scale maps in the coder's latent layout.  band, window_latent: the tensors
 * of sicn_ragged_ctx_roi_move_layout; nothing outside them is written.  status_dev[n_slots], flags_dev[n_slots]: the verdicts and
 * the flag words.  SIX enqueued operations whatever n_slots is, FIVE when no slot has non-anchor capacity. */
int sicn_ragged_ctx_roi_move_decode_async(const sicn_ragged_ctx_roi_move *mv, const int32_t *xy_dev, const uint8_t *containers,
                                          const uint8_t *scales, uint8_t *band, uint8_t *window_latent, sicn_codec_status *status_dev,
                                          uint32_t *flags_dev, void *workspace, size_t workspace_bytes, void *hip_stream);
/* recon: layers 4 .. 7 of the window latents; roi_out: the ROI pixels.  Reads the placement of the last decode_async on the same
 * stream.  ONE launch. */
int sicn_ragged_ctx_roi_move_cut_async(const sicn_ragged_ctx_roi_move *mv, const uint8_t *recon, uint8_t *roi_out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_CTX_ROI_MOVE_H */
