/*
 * sicn_ragged_hyper.h — what the hyperprior configuration needs of a ragged batch (library 0.8, sicn_version() >= 8), on top of
 * sicn_ragged.h: GDN / IGDN layers in a ragged net, and the crop of every image of a ragged tensor in one launch.  With them
 * hyperprior.RaggedHyperpriorCodec runs main transform, hyper stacks, z coder and scale map over images of different sizes with one set
 * of launches per batch (the y coder, rANS-WC, is still one per image).  EXTENSION BEYOND THE REFERENCE, parity unpinned, as sicn_gdn.h.
 * Data model, limits and error codes: sicn_ragged.h.
 */
#ifndef SICN_RAGGED_HYPER_H
#define SICN_RAGGED_HYPER_H

#include "sicn_gdn.h"
#include "sicn_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sicn_ragged_net_create with gdn[i] (NULL entries, or gdn == NULL: the reference ReLU) in place of layer i's ReLU, as
 * sicn_net_create_gdn: gdn[i]'s channel count must equal descs[i].OFM_CH (SICN_EINVAL); the net keeps references to the activations
 * (caller keeps them alive).  sicn_ragged_net_create is the gdn == NULL case.  A tapped layer's output and the chain's last output are the activated bytes.  Any channel count sicn_gdn_create takes. */
int sicn_ragged_net_create_gdn(const sicn_layer_desc *descs, sicn_weights *const *weights, const sicn_gdn *const *gdn, int n_layers,
                               const int32_t *widths, const int32_t *heights, int n_images, sicn_ragged_net **out);

/* ---- ragged crop: image i's [src_h[i]][src_w[i]][channels] array cut to its top-left [dst_h[i]][dst_w[i]][channels] -------------
 * Both tensors are ragged tensors as above (back to back, 64-bit offsets).  A work item is SICN_RAGGED_CROP_ROWS destination rows of
 * one image (the last item of an image holds the rest).  SICN_EINVAL: n_images < 1, channels < 1, a size < 1 or > 2^20, dst larger
 * than src in either dimension of any image, one image's tensor >= 2^31 bytes, >= 2^31 - 1 work items.  Rows are copied as 16-byte
 * vectors where the image's source and destination row bytes, both image offsets and both base pointers are multiples of 16 (every
 * tensor with channels % 16 == 0 on aligned pointers), byte by byte otherwise (RGB: 336-byte rows cut to 300). */
#define SICN_RAGGED_CROP_ROWS 8
typedef struct sicn_ragged_crop sicn_ragged_crop;
/* Pure host, no device.  out[] = { byte offset of `image` in src, in dst, bytes of the whole src tensor, of the whole dst tensor }. */
int sicn_ragged_crop_layout(const int32_t *src_w, const int32_t *src_h, const int32_t *dst_w, const int32_t *dst_h, int channels,
                            int n_images, int image, int64_t out[4]);
/* Uploads its two tables to the current device.  Synchronous.  SICN_ENODEV off gfx950 (after the argument checks). */
int sicn_ragged_crop_create(const int32_t *src_w, const int32_t *src_h, const int32_t *dst_w, const int32_t *dst_h, int channels,
                            int n_images, sicn_ragged_crop **out);
void sicn_ragged_crop_free(sicn_ragged_crop *crop);
/* ONE launch: enqueue only, no allocation, no synchronisation, capturable.  `src` is only read; src and dst must not overlap.
 * SICN_EINVAL (nothing enqueued) for a NULL argument. */
int sicn_ragged_crop_run(const sicn_ragged_crop *crop, const uint8_t *src, uint8_t *dst, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_HYPER_H */
