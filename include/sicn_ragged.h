/*
 * sicn_ragged.h — ragged batches: the layer chain of sicn.h over n images of n DIFFERENT sizes, one kernel launch per layer
 * for the whole batch (library 0.6, sicn_version() >= 6).  Same bytes as sicn_net_forward on every image alone.
 *
 * Data model.  A ragged tensor is the images' [H][W][C] uint8 arrays back to back, no padding between them: image i at layer
 * boundary l starts at byte  off(l, i) = sum over j < i of H(l, j) * W(l, j) * C(l).  Boundary -1 is the chain's input, boundary
 * l >= 0 the output of layer l.  The sizes follow the chain rule of sicn_layer_desc: conv ceil(in / 2), deconv 2 * in (the
 * reconstruction of a 100 x 36 image is 112 x 48).  With equal sizes the layout is the [n][H][W][C] batch of sicn.h, byte for byte.
 * Inner tensors have C % 16 == 0, so every image starts 16-byte aligned when the tensor does; tensors handed to the library must be
 * 16-byte aligned.  One image's slice is a plain contiguous NHWC array: whatever takes one (the coder of sicn_codec.h) takes it; the
 * whole ragged latent (boundary 3) is coded in one go, three launches for the batch, by sicn_ragged_coder_encode_async
 * (sicn_ragged_codec.h, library 0.7).
 *
 * Kernels.  Every layer runs on the channel-generic MFMA kernels ("mfma_conv_any" / "mfma_deconv_any" of sicn.h) in their ragged
 * form: a workgroup is one 16 x 16 tile of positions x 64 output channels of one image and finds that image through tables the net
 * uploads once, at creation.  A layer these kernels do not serve (sicn_kernel_for's width rules: IFM_CH % 32 == 0 and
 * OFM_CH % 16 == 0, both <= 1024, conv 3 -> N, deconv N -> 3) is SICN_EINVAL: the ragged net has no other kernel to fall back on.
 * Since library 0.15 the two RGB shapes, conv 3 -> N and deconv N -> 3, run on packed-K kernels of their own in a net made here; same
 * bytes (sicn_ragged_rgb.h, which also has the entry point that chooses the form and the one that names a layer's kernel).
 *
 * Activations (library 0.8, sicn_version() >= 8; declared in sicn_ragged_hyper.h).  sicn_ragged_net_create_gdn gives layer i the
 * GDN / IGDN of sicn_gdn.h in place of the reference ReLU: the layer kernel stores its pre-activation lanes and the activation
 * rewrites the whole boundary tensor in place, [tensor bytes / OFM_CH positions][OFM_CH] — a ragged tensor is exactly what
 * sicn_gdn_apply takes, so the image tables play no part.  Two launches for such a layer (one more per 2 GiB of tensor), for the
 * whole batch; the bytes are sicn_net_create_gdn's on every image alone.
 *
 * Crop (library 0.8, sicn_ragged_hyper.h).  The chain rule rounds up: a deconv doubles what a conv halved towards the ceiling, so
 * h_s(z) of the hyperprior is 4 * ceil(./4) per image and a reconstruction 16 * ceil(./16).  sicn_ragged_crop_* cuts every image of
 * a ragged tensor to its top-left [dst_h][dst_w][C], one launch for the batch, into another ragged tensor.
 *
 * Limits (SICN_EINVAL): n_images < 1, a width or height < 1 or > 2^20, one image's tensor at any boundary >= 2^31 bytes, a layer
 * with >= 2^31 - 1 work items.  The whole ragged tensor may exceed 2 GiB: offsets are 64-bit.  SICN_ENODEV off gfx950.
 */
#ifndef SICN_RAGGED_H
#define SICN_RAGGED_H

#include "sicn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sicn_ragged_net sicn_ragged_net;

/* Where image `image` sits at layer boundary `layer` (-1: the input; l: the output of layer l), and how layer l is cut into work.
 * Pure host, no device.  The spatial fields of `descs` are ignored (the sizes come from widths[] / heights[]); the channel counts,
 * `transposed`, SIMD, PE and W_TILES are used and checked as in sicn_validate_desc.
 * out[] = { W, H, C, byte offset of the image, bytes of the whole tensor of that boundary, first work item of the image in layer l,
 *           tiles_x of the image in layer l, work items of layer l over all images }.
 * A work item is one 16 x 16 tile of the layer's M grid (conv: output pixels; deconv: input pixels, times 4 phases, the phase in
 * the low two bits); the last three fields are 0 for layer = -1.  They describe the channel-generic cut; the cut a net with packed
 * RGB ends launches is sicn_ragged_rgb_layout's (sicn_ragged_rgb.h). */
int sicn_ragged_layout(const sicn_layer_desc *descs, int n_layers, const int32_t *widths, const int32_t *heights, int n_images,
                       int layer, int image, int64_t out[8]);

/* widths[i] x heights[i]: the size of image i at the chain's input.  The net keeps references to `weights` (caller keeps them
 * alive) and owns its lookup tables on the current device.  Synchronous. */
int sicn_ragged_net_create(const sicn_layer_desc *descs, sicn_weights *const *weights, int n_layers, const int32_t *widths,
                           const int32_t *heights, int n_images, sicn_ragged_net **out);
void sicn_ragged_net_free(sicn_ragged_net *net);
/* Two ping-pong buffers, each the largest tensor between two layers (no device is needed to ask). */
size_t sicn_ragged_net_workspace_bytes(const sicn_ragged_net *net);
/* Layers [first_layer, last_layer] over the whole batch: `in` is the ragged tensor of boundary first_layer - 1, `out` that of
 * boundary last_layer, `tap_out` (tap_layer >= 0) that of boundary tap_layer.  The contract of sicn_net_forward: enqueue only, no
 * allocation, no synchronisation, capturable into a hipGraph, one call in flight per workspace; `tap_out` must not overlap `in`,
 * `out` or the workspace.  SICN_ENOSPC (nothing enqueued) when the workspace is too small. */
int sicn_ragged_net_forward(const sicn_ragged_net *net, int first_layer, int last_layer, const uint8_t *in, uint8_t *out,
                            int tap_layer, uint8_t *tap_out, void *workspace, size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_H */
