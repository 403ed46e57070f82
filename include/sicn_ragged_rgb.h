/*
 * sicn_ragged_rgb.h — ragged nets: packed-K kernels for the RGB ends of a chain (library 0.15, sicn_version() >= 15).
 *
 * The ragged kernels of sicn_ragged.h run a conv 3 -> N and a deconv N -> 3 in the zero-padded form of the channel-generic family:
 * the conv walks 25 K steps of 64 bytes of which 3 bytes are real, the deconv runs one workgroup per phase, each staging the patch
 * again and multiplying a 16-row tile of which 3 rows are real.  A net created here with SICN_RAGGED_RGB_PACKED runs those two
 * layer shapes on kernels of their own ("mfma_conv_rgb_packed", "mfma_deconv_rgb_packed"):
 *   conv 3 -> N   (N % 16 == 0, N <= 1024)  one 16 x 16 tile of output positions per work item, as before; the patch is expanded to
 *                 RGBX once per workgroup and K is one 32-byte group per kernel row — 3 K steps where there were 25; the blocks of
 *                 64 output channels are a loop inside the workgroup, not grid.y
 *   deconv N -> 3 (N % 32 == 0, N <= 1024)  one 16 x 16 tile of INPUT positions with all four phases per work item — a quarter of
 *                 the items; the patch of a K chunk is staged once per tile and nine tap offsets replace the 9 + 6 + 6 + 4 taps of
 *                 the four phases, with 12 real rows of 16 where there were 3
 * Every other layer, every tensor, every offset and every byte is what sicn_ragged.h says: the two forms of a net differ in time
 * only.  The weight images of the packed kernels are packed at net creation from the weights' plain copy and owned by the net.
 * A conv 3 -> N reads its input as aligned 4-byte words: the input tensor must be 4-byte aligned (sicn_ragged.h asks for 16) and
 * up to 3 bytes behind its last byte, to the next multiple of 4, are read (and ignored) — the allowance "l0_rgb" of sicn.h takes.
 *
 * sicn_ragged_net_create and sicn_ragged_net_create_gdn make PACKED nets since library 0.15.
 */
#ifndef SICN_RAGGED_RGB_H
#define SICN_RAGGED_RGB_H

#include "sicn_gdn.h"
#include "sicn_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SICN_RAGGED_RGB_GENERIC 0   /* every layer on the channel-generic ragged kernels */
#define SICN_RAGGED_RGB_PACKED 1    /* conv 3 -> N and deconv N -> 3 on the packed-K kernels, every other layer unchanged */

/* sicn_ragged_net_create_gdn (sicn_ragged_hyper.h; gdn may be NULL: sicn_ragged_net_create) with the form of the RGB ends.
 * Any other rgb_ends: SICN_EINVAL. */
int sicn_ragged_net_create_rgb(const sicn_layer_desc *descs, sicn_weights *const *weights, const sicn_gdn *const *gdn, int n_layers,
                               const int32_t *widths, const int32_t *heights, int n_images, int rgb_ends, sicn_ragged_net **out);

/* The kernel layer `layer` of the net runs on: "mfma_conv_any", "mfma_deconv_any", "mfma_conv_rgb_packed" or
 * "mfma_deconv_rgb_packed" (static strings).  NULL for a null net or a layer out of range. */
const char *sicn_ragged_net_kernel_for(const sicn_ragged_net *net, int layer);

/* How a net of form rgb_ends cuts layer `layer` into work.  Pure host; arguments and checks as sicn_ragged_layout (layer >= 0).
 * out[] = { first work item of the image, tiles_x of the image, work items of the layer over all images }.
 * GENERIC: sicn_ragged_layout's out[5 .. 7].  PACKED: a deconv N -> 3 has ONE item per 16 x 16 tile of input positions (a quarter
 * of the generic items); every other layer as GENERIC. */
int sicn_ragged_rgb_layout(const sicn_layer_desc *descs, int n_layers, const int32_t *widths, const int32_t *heights, int n_images,
                           int rgb_ends, int layer, int image, int64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_RGB_H */
