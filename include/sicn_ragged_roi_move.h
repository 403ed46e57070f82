/*
 * sicn_ragged_roi_move.h — the ROI decode of sicn_ragged_window.h with rectangles that MOVE: their positions are read from device
 * memory on every call (library 0.17, sicn_version() >= 17).  Nothing in the container format, in the archive or in any existing
 * symbol changes.  The rANS-W configuration (mode 3); the hyperprior configuration follows separately.
 *
 * Why.  sicn_ragged_window_create, the two sicn_ragged_cut_create and the window's ragged net are made for exactly one set of
 * rectangles: device allocations, synchronous uploads and, when they go, frees that synchronise the device.  A viewer that pans or a
 * loader that draws crops pays all of that per rectangle.  Here the objects are made ONCE for a list of SLOTS, and a call costs its
 * launches alone.
 *
 * Slots.  A slot is { image, w, h }: a pixel rectangle of fixed size w x h that looks into `image` of the coder's batch.  Several
 * slots may name one image, in any order — two details of one photograph are two slots of one call.  What moves is the slot's
 * position (x0, y0), an int32 pair in device memory, read when the kernels run: a captured graph replays with new positions.
 *
 * Capacity (pure host, sicn_ragged_roi_move_capacity).  cw_cap is the largest cw that sicn_ragged_roi_plan gives over all positions
 * x0 in [0, image_w - w] of a rectangle of width w BEFORE its clip to the latent,
 *     cw(x0) = ceil((x0 + w + margin_hi) / 2^L) - floor((x0 - margin_lo) / 2^L),
 * which has the period 2^L in x0 (the first min(image_w - w, 2^L - 1) + 1 positions decide it) and is at most floor((w + 75) / 16) for
 * L = 4; that value is then clipped to lat_w.  rh_cap likewise from h, image_h, lat_h.
 *
 * Placement (pure host, sicn_ragged_roi_move_place; the device states the same rule, csrc/roi_move_host.hpp).  For a position (x0, y0):
 *   1. x0 is clamped into [0, image_w - w], y0 into [0, image_h - h];
 *   2. if either moved, bit 0 (SICN_ROI_MOVE_CLAMPED) of the slot's flag word is set, else the word is 0: the flag is deterministic,
 *      and nothing can be addressed out of bounds from device data;
 *   3. c0 = min(plan.c0, lat_w - cw_cap), r0 = min(plan.r0, lat_h - rh_cap), plan = sicn_ragged_roi_plan of the clamped rectangle;
 *   4. the corner inside the window's reconstruction is x = x0 - 2^L c0, y = y0 - 2^L r0.
 * The placed window [c0, c0 + cw_cap) x [r0, r0 + rh_cap) contains the planned one and reaches the latent's edge wherever the planned
 * one did, so the margins of sicn_ragged_window.h hold and the bytes are those of the full decode, cut to the rectangle.
 *
 * Layout (pure host, sicn_ragged_roi_move_layout; L = 4).  Per slot, with R = lat_w * lat_c and wss its image's stream length:
 *   max_streams = min(n_streams, ceil(rh_cap R / wss) + 1) work items, a fixed range of the decode grid;
 *   a band of max_streams * wss bytes at band_offset (64-bit, a multiple of 16): the streams [first_stream, end_stream) that hold
 *     the rows [r0, r0 + rh_cap) land at its start, as in sicn_ragged_window.h;
 *   its window latent [rh_cap][cw_cap][lat_c], its reconstruction [16 rh_cap][16 cw_cap][3] and its pixels [h][w][3], each back to
 *     back in slot order in its ragged tensor — the layouts of a ragged net made for the sizes (16 cw_cap, 16 rh_cap);
 *   a workspace block of its own with the layout its image has in the full coder: two slots of one image share nothing writable.
 *
 * The chain, NINE launches whatever n_slots is, linear (a captured graph of it has no parallel branches):
 *   sicn_ragged_roi_move_decode_async   4: placement (k_roi_place: a few words per slot) -> the selected streams of every slot ->
 *                                          one verdict per slot -> the window latents
 *   sicn_ragged_net_forward 4 .. 7      4: a ragged net made for the sizes (16 cw_cap, 16 rh_cap)
 *   sicn_ragged_roi_move_cut_async      1: the rectangles out of the reconstructions -> the ROI pixels
 *
 * Verdicts.  status_dev[n_slots]: those of sicn_ragged_window_decode_async for the slot's image and the streams the slot selected
 * in THIS call; bit 7 is never set; .bytes = the symbols of the selected streams.  A slot's verdict concerns that slot alone.
 *
 * One call in flight per object (the placement writes the object's own device tables) and per workspace.
 *
 * Limits (SICN_EINVAL): n_slots < 1, an image index out of range, w or h < 1 or larger than the image, an image without a size or
 * larger than 16 x its latent, the limits of sicn_ragged_codec_layout and sicn_ragged_cut_layout (a reconstruction of 2^31 bytes,
 * 2^31 - 1 work items).  SICN_ENODEV off gfx950 (creation and the asynchronous calls).
 */
#ifndef SICN_RAGGED_ROI_MOVE_H
#define SICN_RAGGED_ROI_MOVE_H

#include "sicn_ragged_window.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SICN_ROI_MOVE_CLAMPED 1u        /* flag bit 0: the position lay outside [0, image - size] and was clamped */
#define SICN_ROI_MOVE_UP_LAYERS 4       /* the layout, the object and the kernels: the eight-layer chain */

typedef struct sicn_ragged_roi_move sicn_ragged_roi_move;

typedef struct sicn_ragged_roi_slot {
    int32_t image, w, h;
} sicn_ragged_roi_slot;

/* Where a slot's rectangle of size w x h at (x0, y0) is placed. */
typedef struct sicn_ragged_roi_placed {
    int32_t x0, y0;                 /* the position after the clamp */
    int32_t c0, r0, cw, rh;         /* the placed latent window: cw = cw_cap, rh = rh_cap */
    int32_t x, y;                   /* the rectangle's corner inside the window's reconstruction */
    uint32_t flags;                 /* SICN_ROI_MOVE_CLAMPED or 0 */
} sicn_ragged_roi_placed;

/* Where a slot lies in the tensors of the chain. */
typedef struct sicn_ragged_roi_move_slot {
    uint64_t band_offset;           /* a multiple of 16; the band's capacity is max_streams * stream_symbols bytes */
    uint64_t latent_offset;         /* [rh_cap][cw_cap][lat_c] in the window latents */
    uint64_t recon_offset;          /* [16 rh_cap][16 cw_cap][3] in the reconstructions */
    uint64_t roi_offset;            /* [h][w][3] in the ROI pixels */
    uint64_t workspace_offset;
    uint32_t cw_cap, rh_cap;
    uint32_t max_streams, first_item;
} sicn_ragged_roi_move_slot;

/* Pure host, no device.  n_up_layers 1 .. 12.  cap[2] out: { cw_cap, rh_cap }.  SICN_EINVAL: a size < 1, w or h larger than the
 * image, the image larger than lat << n_up_layers, NULL. */
int sicn_ragged_roi_move_capacity(int n_up_layers, int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, int32_t w, int32_t h,
                                  int32_t cap[2]);
/* Pure host, no device.  Any int32 position is admissible: it is clamped.  SICN_EINVAL as above. */
int sicn_ragged_roi_move_place(int n_up_layers, int32_t image_w, int32_t image_h, int32_t lat_w, int32_t lat_h, int32_t w, int32_t h,
                               int32_t x0, int32_t y0, sicn_ragged_roi_placed *out);

/* Pure host, no device.  The first five arguments as in sicn_ragged_codec_layout; image_w / image_h: [n_images] pixels.
 * slots_out_or_null: [n_slots].  totals[6] out: bytes of the band tensor, of the window latents, of the reconstructions, of the ROI
 * pixels and of the workspace, and the work items of the decode grid. */
int sicn_ragged_roi_move_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                                const uint32_t *image_w, const uint32_t *image_h, int n_images, const sicn_ragged_roi_slot *slots,
                                int n_slots, sicn_ragged_roi_move_slot *slots_out_or_null, uint64_t totals[6]);

/* Over an existing coder made WITH image sizes, which must outlive the object.  Allocates and uploads its tables on the current
 * device, once.  Synchronous. */
int sicn_ragged_roi_move_create(const sicn_ragged_coder *coder, const sicn_ragged_roi_slot *slots, int n_slots, sicn_ragged_roi_move **out);
void sicn_ragged_roi_move_free(sicn_ragged_roi_move *mv);
size_t sicn_ragged_roi_move_workspace_bytes(const sicn_ragged_roi_move *mv);

/* The family's contract: enqueue only, no allocation, no host synchronisation, capturable into a hipGraph; SICN_EINVAL (NULL, a
 * workspace that is not 16-byte aligned, positions that are not 4-byte aligned) and SICN_ENOSPC (a workspace smaller than
 * sicn_ragged_roi_move_workspace_bytes) before any launch.  xy_dev: [n_slots] pairs { x0, y0 } in device memory, read when the
 * kernels run.  containers / valid_dev_or_null: the coder's slot buffer and valid array (indexed by IMAGE).  band, window_latent:
 * the tensors of sicn_ragged_roi_move_layout; a band byte outside the symbols this call selects is not written.  status_dev
 * [n_slots], flags_dev[n_slots]: the verdicts and the flag words.  FOUR launches whatever n_slots is. */
int sicn_ragged_roi_move_decode_async(const sicn_ragged_roi_move *mv, const int32_t *xy_dev, const uint8_t *containers,
                                      const sicn_codec_status *valid_dev_or_null, uint8_t *band, uint8_t *window_latent,
                                      sicn_codec_status *status_dev, uint32_t *flags_dev, void *workspace, size_t workspace_bytes,
                                      void *hip_stream);
/* recon: layers 4 .. 7 of the window latents; roi_out: the ROI pixels.  Reads the placement of the last decode_async on the same
 * stream.  ONE launch.  The same contract. */
int sicn_ragged_roi_move_cut_async(const sicn_ragged_roi_move *mv, const uint8_t *recon, uint8_t *roi_out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_ROI_MOVE_H */
