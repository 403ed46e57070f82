/*
 * sicn_ragged_rect.h — ragged nets: the last layer stores a RECTANGLE of every reconstruction, in either pixel layout, at an origin
 * that may be read from device memory when the kernel runs.
 * sicn_version() stays 17: these symbols being present is the marker.
 *
 * A net created here ends with a deconv N -> 3 whose epilogue stores, of image i's reconstruction (OH_i x OW_i by the chain rule),
 * the pixels of rectangle (x0_i, y0_i, w_i, h_i) and nothing else:
 *   - boundary n - 1 holds image i as [h_i][w_i][3] (INTERLEAVED out) or as three planes [3][h_i][w_i] (PLANAR out) of uint8; the
 *     images back to back, image i at byte 3 * sum_{j < i} h_j w_j, no padding and no alignment between them
 *   - output pixel (oy, ox) is stored iff 0 <= oy - y0 < h and 0 <= ox - x0 < w, at the address its in-rectangle coordinates
 *     (oy - y0, ox - x0) give.  The sizes are the creation's; the address is formed from the in-rectangle coordinates alone, so no
 *     store lands outside the image's own 3 h_i w_i bytes WHATEVER the origin is
 *   - the creation's origins lie inside the reconstruction.  sicn_ragged_net_forward_at reads the origins from the caller's device
 *     array instead: every int32 pair is admissible there.  Where a rectangle reaches outside the reconstruction, the bytes out
 *     there are NOT WRITTEN (they keep what the tensor held); the bytes inside are those of the full reconstruction
 *   - a workgroup whose 32 x 32 output pixels do not meet its image's rectangle returns before it loads anything: no recon tensor,
 *     no cut launch, and the tiles around the rectangle cost a table look-up
 * Every other boundary, tap and byte is what it is without this header.  The kernels are "mfma_deconv_rgb_rect" and
 * "mfma_deconv_rgb_planar_rect": the packed-K deconv of sicn_ragged_rgb.h with another epilogue.
 */
#ifndef SICN_RAGGED_RECT_H
#define SICN_RAGGED_RECT_H

#include "sicn_ragged_ctx_roi_move.h"
#include "sicn_ragged_planar.h"
#include "sicn_ragged_roi_move.h"
#include "sicn_ragged_window.h"   /* sicn_ragged_rect */

#ifdef __cplusplus
extern "C" {
#endif

/* sicn_ragged_net_create_planar with rectangles in place of output sizes: rects[i] = (x0, y0, w, h) of image i's reconstruction, the
 * layout of boundary n - 1 according to pixels_out.  rects == NULL: sicn_ragged_net_create_planar without sizes.  SICN_EINVAL, with
 * nothing created, for:
 *   - a last layer that is not a deconv N -> 3
 *   - rgb_ends != SICN_RAGGED_RGB_PACKED
 *   - a GDN / IGDN on the last layer
 *   - a rectangle with w < 1 or h < 1, with x0 < 0 or y0 < 0, or one that reaches beyond the chain-rule size
 * and whatever sicn_ragged_net_create_planar refuses. */
int sicn_ragged_net_create_rect(const sicn_layer_desc *descs, sicn_weights *const *weights, const sicn_gdn *const *gdn, int n_layers,
                                const int32_t *widths, const int32_t *heights, int n_images, int rgb_ends, int pixels_in, int pixels_out,
                                const sicn_ragged_rect *rects, sicn_ragged_net **out);

/* Where image `image` lies at boundary n - 1 of such a net.  Pure host; the refusals of sicn_ragged_net_create_rect that concern the
 * chain and the rectangles (rects == NULL: the whole reconstructions).
 * out[] = { w, h, byte offset of the image, bytes of the whole tensor, the image's LIVE tiles in the last layer at the creation's
 * origin: those of its 16 x 16 tiles of input positions whose 32 x 32 output pixels meet the rectangle }. */
int sicn_ragged_rect_layout(const sicn_layer_desc *descs, int n_layers, const int32_t *widths, const int32_t *heights, int n_images,
                            const sicn_ragged_rect *rects, int image, int64_t out[5]);

/* sicn_ragged_net_forward with the rectangles' origins read from origins_dev: int32 [n_images][2] = (x0, y0) per image, 4-byte
 * aligned device memory, read when the last layer's kernel runs.  The sizes and offsets stay the creation's.  NULL: the creation's
 * origins; sicn_ragged_net_forward of a net made with rectangles is this call with NULL.  SICN_EINVAL for non-NULL origins on a net
 * not made with rectangles, with last_layer != n_layers - 1, or at a misaligned address.  tap_out at tap_layer == n_layers - 1 is
 * laid out as `out` is.  Enqueue only, nothing allocated, capturable. */
int sicn_ragged_net_forward_at(const sicn_ragged_net *net, int first_layer, int last_layer, const uint8_t *in, uint8_t *out, int tap_layer,
                               uint8_t *tap_out, void *workspace, size_t workspace_bytes, const int32_t *origins_dev, void *hip_stream);

/* The moving ROI decodes (sicn_ragged_roi_move.h, sicn_ragged_ctx_roi_move.h) as a source of origins: the device pointer to
 * int32 [n_slots][2], the placed rectangle's corner (x, y) inside its window reconstruction, which the object's place kernel
 * rewrites on every decode_async and which holds the placement of (0, 0) before the first.  Owned by the object; handed to
 * sicn_ragged_net_forward_at of a window net made with the rectangles (0, 0, w, h) of the slots, layer 7 stores the ROI pixels
 * themselves and the cut_async pass is not needed.  NULL for a NULL object. */
const int32_t *sicn_ragged_roi_move_origins(const sicn_ragged_roi_move *mv);
const int32_t *sicn_ragged_ctx_roi_move_origins(const sicn_ragged_ctx_roi_move *mv);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_RECT_H */
