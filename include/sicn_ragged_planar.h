/*
 * sicn_ragged_planar.h — ragged nets: planar RGB at the two pixel boundaries, the output at sizes of the caller's choice.
 * sicn_version() stays 17: these symbols being present is the marker.
 *
 * The RGB boundaries of sicn_ragged.h are pixel-interleaved: [h][w][3] per image, the images back to back.  A net created here may
 * read its input, write its output, or both, as PLANAR RGB instead:
 *   - image i is three planes [3][h_i][w_i] of uint8, R then G then B; planes back to back, images back to back, no padding and no
 *     alignment between them
 *   - image i starts at byte 3 * sum_{j < i} h_j w_j — the offset it has in the interleaved tensor of the same sizes, so
 *     sicn_ragged_layout's offsets of boundary -1 stay true
 *   - input (boundary -1 of a chain whose layer 0 is a conv 3 -> N): h_i x w_i are the images' sizes
 *   - output (boundary n - 1 of a chain whose last layer is a deconv N -> 3): h_i x w_i are the OUTPUT SIZES given at creation, each
 *     at least 1 and at most the chain-rule size OH_i x OW_i of that boundary.  The tensor holds the top-left h_i x w_i pixels of each
 *     reconstruction; the pixels outside are computed and not stored.  NULL sizes mean the chain-rule sizes.
 * The alignment rules are those of sicn_ragged_rgb.h: the input tensor is 4-byte aligned, it is read as aligned 4-byte words, and no
 * load touches a byte before its first one or beyond its size rounded up to a multiple of 4.  The output is written with stores
 * that touch the image's own bytes only.
 * Every inner boundary, the latent, every tap of an inner layer, every coder and every archive byte are what they are without this
 * header.  The planar ends run on kernels of their own ("mfma_conv_rgb_planar", "mfma_deconv_rgb_planar"): the packed-K kernels of
 * sicn_ragged_rgb.h with another loader and another epilogue.  The channel-generic form of the RGB ends has no planar sibling.
 */
#ifndef SICN_RAGGED_PLANAR_H
#define SICN_RAGGED_PLANAR_H

#include "sicn_ragged_rgb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SICN_RAGGED_PIXELS_INTERLEAVED 0   /* [h][w][3] */
#define SICN_RAGGED_PIXELS_PLANAR 1        /* [3][h][w] */

/* sicn_ragged_net_create_rgb with the pixel layout of the input (pixels_in) and of the output (pixels_out), and the output sizes
 * out_widths / out_heights (one per image, or both NULL: the chain-rule sizes).  With both layouts INTERLEAVED and no sizes it IS
 * sicn_ragged_net_create_rgb.  SICN_EINVAL, with nothing created, for:
 *   - a pixels_* value other than the two
 *   - PLANAR in on a chain whose layer 0 is not a conv 3 -> N; PLANAR out on a chain whose last layer is not a deconv N -> 3
 *   - PLANAR with rgb_ends != SICN_RAGGED_RGB_PACKED
 *   - PLANAR out on a last layer that carries a GDN / IGDN (the activation walks [positions][C])
 *   - out_widths / out_heights with INTERLEAVED out, or only one of the two
 *   - an output size below 1 or above the chain-rule size
 * and whatever sicn_ragged_net_create_rgb refuses.
 * sicn_ragged_net_forward of such a net reads `in` as planar when first_layer == 0 (planar in), writes `out` as planar when
 * last_layer == n_layers - 1 and `tap_out` as planar when tap_layer == n_layers - 1 (planar out); every other tensor is unchanged. */
int sicn_ragged_net_create_planar(const sicn_layer_desc *descs, sicn_weights *const *weights, const sicn_gdn *const *gdn, int n_layers,
                                  const int32_t *widths, const int32_t *heights, int n_images, int rgb_ends, int pixels_in, int pixels_out,
                                  const int32_t *out_widths, const int32_t *out_heights, sicn_ragged_net **out);

/* Where image `image` lies at the two pixel boundaries.  Pure host; descs .. n_images as sicn_ragged_layout, pixels_out, out_widths
 * and out_heights as above (the same refusals).
 * out[] = { w, h, byte offset of the image, bytes of the whole tensor } of the OUTPUT boundary n - 1 — with INTERLEAVED out the
 * chain-rule sizes and sicn_ragged_layout's offsets — then { byte offset of the image, bytes of the whole tensor } of the INPUT
 * boundary -1, which are the same in both layouts. */
int sicn_ragged_planar_layout(const sicn_layer_desc *descs, int n_layers, const int32_t *widths, const int32_t *heights, int n_images,
                              int pixels_out, const int32_t *out_widths, const int32_t *out_heights, int image, int64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_PLANAR_H */
