// Ragged batches (include/sicn_ragged.h, _hyper.h): the channel-generic MFMA kernels of k_mfma16c.hip over n images of n different sizes,
// one launch per layer for the whole batch.  The tile body is any_tile() (k_any_body.hpp), the weight image is pack_any()'s; what
// is new is how a workgroup finds its image.
//
// Grid: x = the layer's work items over all images (a work item = one 16 x 16 tile of one image's M grid; the deconv has 4 per tile,
// the phase in the low two bits), y = blocks of 64 output channels, z = 1.  Two tables per layer, built on the host at net creation:
//   tile_image[tile]  : the image a tile belongs to (one entry per tile, not per phase) — ONE load resolves item -> image
//   rows[image]       : { IW, IH, OW, OH, tiles_x, first_item, in_off, out_off }, the image's sizes in this layer, its first work item
//                       and its 64-bit byte offsets in the layer's input and output tensors
// Both loads are wave-uniform (they depend on blockIdx.x only) and stay in scalar registers.
//
// The RGB ends (conv 3 -> N, deconv N -> 3) of a SICN_RAGGED_RGB_PACKED net (include/sicn_ragged_rgb.h) run on the kernels of
// k_ragged_rgb.hip with the same two tables; the deconv N -> 3 is then cut into one item per tile, all four phases (ragged_plan).
//
// A layer with a GDN / IGDN (sicn_ragged_net_create_gdn) runs the same kernel with ACT_FLOOR_RAW and then the activation of k_gdn.hip in
// place over the whole boundary tensor: [bytes / OFM_CH][OFM_CH], no table needed.  The ragged crop at the end of this file is the cut
// of k_ragged_window.hip at the corner of every image: the rectangles (0, 0, dst_w, dst_h), the images back to back, the same handle.
//
// A net with PLANAR pixels (include/sicn_ragged_planar.h) runs the planar siblings of the packed RGB kernels at the boundary that is
// planar; a planar output has sizes of its own (planar_out_plan), which reach the kernel through the PlanarOut table.
//
// A net with RECTANGLES (include/sicn_ragged_rect.h) runs the deconv N -> 3 with the rectangle epilogue in either layout: the sizes
// and offsets through the same PlanarOut table, the origins through an int32 [n_images][2] table of the net's or the caller's.
#include <new>
#include <vector>

#include "../../include/sicn_ragged_hyper.h"
#include "../../include/sicn_ragged_planar.h"
#include "../../include/sicn_ragged_rect.h"
#include "../../include/sicn_ragged_rgb.h"
#include "../../include/sicn_ragged_window.h"
#include "device_table.hpp"
#include "k_any_body.hpp"
#include "k_ragged_common.hpp"
#include "ragged_planar_host.hpp"
#include "ragged_rect_host.hpp"
#include "ragged_rgb_host.hpp"
#include "sicn_gdn_internal.h"

namespace sicn {

template <bool DECONV, int NT>
__global__ __launch_bounds__(256) void k_any_ragged(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const int8_t *__restrict__ wimg,
                                                    const int8_t *__restrict__ bias, const RaggedRow *__restrict__ rows,
                                                    const uint32_t *__restrict__ tile_image, int C, int O, uint32_t floor2)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int item = (int)blockIdx.x;
    const int img = __builtin_amdgcn_readfirstlane((int)tile_image[DECONV ? item >> 2 : item]);
    const RaggedRow *row = rows + img;
    const int IW = __builtin_amdgcn_readfirstlane(row->IW), IH = __builtin_amdgcn_readfirstlane(row->IH);
    const int OW = __builtin_amdgcn_readfirstlane(row->OW), OH = __builtin_amdgcn_readfirstlane(row->OH);
    const int tiles_x = __builtin_amdgcn_readfirstlane(row->tiles_x);
    int local = item - __builtin_amdgcn_readfirstlane(row->first_item), qy = 0, qx = 0;
    const uint64_t in_off = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)row->in_off) |
                            (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(row->in_off >> 32)) << 32;
    const uint64_t out_off = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)row->out_off) |
                             (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(row->out_off >> 32)) << 32;
    if (DECONV) {
        qy = (local >> 1) & 1;
        qx = local & 1;
        local >>= 2;
    }
    const int ty = local / tiles_x, tx = local - ty * tiles_x;
    any_tile<DECONV, NT>(in + in_off, out + out_off, wimg, bias, IW, IH, C, OW, OH, O, ty * ANY_T, tx * ANY_T, qy, qx, (int)blockIdx.y,
                         floor2, smem);
}

// ---- the layout of a ragged chain: pure host ----------------------------------------------------------------------------------
struct RaggedBoundary {                     // one layer boundary: -1 (index 0) = the input, l (index l + 1) = the output of layer l
    int C;
    std::vector<int32_t> W, H;
    std::vector<int64_t> off;               // [n_images + 1]: byte offsets, the last one = the tensor's bytes
};
struct RaggedLayerPlan {
    bool packed = false;                    // an RGB end on the packed-K kernels (k_ragged_rgb.hip)
    int per_tile = 1;                       // work items per 16 x 16 tile: the deconv's four phases, except in its packed form
    std::vector<int32_t> tiles_x;
    std::vector<int64_t> first_item;        // [n_images + 1]: the last one = the layer's work items
};
struct RaggedPlan {
    std::vector<RaggedBoundary> bounds;     // [n_layers + 1]
    std::vector<RaggedLayerPlan> layers;    // [n_layers]
};

static int ragged_plan(const sicn_layer_desc *descs, int n_layers, const int32_t *widths, const int32_t *heights, int n_images,
                       int rgb_ends, RaggedPlan *plan)
{
    if (rgb_ends != SICN_RAGGED_RGB_GENERIC && rgb_ends != SICN_RAGGED_RGB_PACKED) return SICN_EINVAL;
    if (!descs || !widths || !heights || n_layers <= 0 || n_layers > 64 || n_images < 1) return SICN_EINVAL;
    for (int i = 0; i < n_images; i++)
        if (widths[i] < 1 || heights[i] < 1 || widths[i] > (1 << 20) || heights[i] > (1 << 20)) return SICN_EINVAL;
    try {
        plan->bounds.assign((size_t)n_layers + 1, RaggedBoundary{});
        plan->layers.assign((size_t)n_layers, RaggedLayerPlan{});
        RaggedBoundary &b0 = plan->bounds[0];
        b0.C = descs[0].IFM_CH;
        b0.W.assign(widths, widths + n_images);
        b0.H.assign(heights, heights + n_images);
        for (int l = 0; l < n_layers; l++) {
            // the descriptor's own checks, on the sizes of image 0 (the spatial fields the caller passed are ignored)
            const RaggedBoundary &bi = plan->bounds[(size_t)l];
            sicn_layer_desc d = descs[l];
            const bool tr = d.transposed == 1;
            d.IFM_ROW = bi.W[0];
            d.IFM_COL = bi.H[0];
            d.OFM_ROW = tr ? 2 * bi.W[0] : (bi.W[0] + 1) / 2;
            d.OFM_COL = tr ? 2 * bi.H[0] : (bi.H[0] + 1) / 2;
            if (int rc = sicn_validate_desc(&d)) return rc;
            if (l > 0 && d.IFM_CH != descs[l - 1].OFM_CH) return SICN_EINVAL;
            if (!any_supported(d.IFM_CH, d.OFM_CH, d.transposed)) return SICN_EINVAL;   // no other kernel to fall back on
            RaggedBoundary &bo = plan->bounds[(size_t)l + 1];
            RaggedLayerPlan &lp = plan->layers[(size_t)l];
            bo.C = d.OFM_CH;
            lp.packed = rgb_ends == SICN_RAGGED_RGB_PACKED && ragged_rgb_packed_serves(d.IFM_CH, d.OFM_CH, d.transposed);
            lp.per_tile = tr && !lp.packed ? 4 : 1;
            bo.W.resize((size_t)n_images);
            bo.H.resize((size_t)n_images);
            lp.tiles_x.resize((size_t)n_images);
            lp.first_item.assign((size_t)n_images + 1, 0);
            for (int i = 0; i < n_images; i++) {
                const int64_t iw = bi.W[(size_t)i], ih = bi.H[(size_t)i];
                const int64_t ow = tr ? 2 * iw : (iw + 1) / 2, oh = tr ? 2 * ih : (ih + 1) / 2;
                if (iw > (1 << 20) || ih > (1 << 20)) return SICN_EINVAL;
                if (ih * iw * d.IFM_CH >= (int64_t)OOB || oh * ow * d.OFM_CH >= (int64_t)OOB) return SICN_EINVAL;   // launch_any's limit
                bo.W[(size_t)i] = (int32_t)ow;
                bo.H[(size_t)i] = (int32_t)oh;
                const int64_t mw = tr ? iw : ow, mh = tr ? ih : oh;
                const int64_t tx = (mw + ANY_T - 1) / ANY_T, ty = (mh + ANY_T - 1) / ANY_T;
                lp.tiles_x[(size_t)i] = (int32_t)tx;
                lp.first_item[(size_t)i + 1] = lp.first_item[(size_t)i] + tx * ty * lp.per_tile;
                if (lp.first_item[(size_t)i + 1] >= RAGGED_MAX_ITEMS) return SICN_EINVAL;
            }
        }
        for (RaggedBoundary &b : plan->bounds) {
            b.off.assign((size_t)n_images + 1, 0);
            for (int i = 0; i < n_images; i++) b.off[(size_t)i + 1] = b.off[(size_t)i] + (int64_t)b.H[(size_t)i] * b.W[(size_t)i] * b.C;
        }
    } catch (const std::bad_alloc &) { return SICN_ENOMEM; }
    return SICN_OK;
}

// The output boundary as a net with `pixels_out` lays it out: per image its size and byte offset, and the tensor's bytes.
// INTERLEAVED: the chain-rule sizes, the plan's offsets; sizes of the caller's are refused.  PLANAR: ow x oh (both NULL: the
// chain-rule sizes), each within [1, chain-rule size], three planes per image back to back; the last layer must be a deconv N -> 3.
static int planar_out_plan(const RaggedPlan &plan, const sicn_layer_desc *descs, int n_layers, int n_images, int pixels_out,
                           const int32_t *ow, const int32_t *oh, std::vector<PlanarOut> *cuts, int64_t *bytes)
{
    if (pixels_out != SICN_RAGGED_PIXELS_INTERLEAVED && pixels_out != SICN_RAGGED_PIXELS_PLANAR) return SICN_EINVAL;
    if ((ow == nullptr) != (oh == nullptr)) return SICN_EINVAL;
    const bool planar = pixels_out == SICN_RAGGED_PIXELS_PLANAR;
    if (!planar && ow) return SICN_EINVAL;
    const sicn_layer_desc &d = descs[n_layers - 1];
    if (planar && !(d.transposed == 1 && d.OFM_CH == 3)) return SICN_EINVAL;
    const RaggedBoundary &b = plan.bounds[(size_t)n_layers];
    cuts->resize((size_t)n_images);
    int64_t off = 0;
    for (int i = 0; i < n_images; i++) {
        const int32_t w = ow ? ow[i] : b.W[(size_t)i], h = oh ? oh[i] : b.H[(size_t)i];
        if (w < 1 || h < 1 || w > b.W[(size_t)i] || h > b.H[(size_t)i]) return SICN_EINVAL;
        (*cuts)[(size_t)i] = PlanarOut{w, h, off};
        off += (int64_t)h * w * b.C;
    }
    *bytes = off;
    return SICN_OK;
}

// The output boundary of a net with rectangles: per image the rectangle's size and the byte offset of its 3 h w bytes (the same in
// both layouts), the origins (x0, y0) back to back, the tensor's bytes and, where asked for, the live tiles per image.  The last layer
// must be a deconv N -> 3 on the packed kernels without an activation of its own; a rectangle lies inside its reconstruction.
static int rect_out_plan(const RaggedPlan &plan, const sicn_layer_desc *descs, int n_layers, int n_images, int pixels_out,
                         const sicn_ragged_rect *rects, std::vector<PlanarOut> *cuts, std::vector<int32_t> *origins, int64_t *bytes,
                         std::vector<int64_t> *live)
{
    if (pixels_out != SICN_RAGGED_PIXELS_INTERLEAVED && pixels_out != SICN_RAGGED_PIXELS_PLANAR) return SICN_EINVAL;
    const sicn_layer_desc &d = descs[n_layers - 1];
    if (!(d.transposed == 1 && d.OFM_CH == 3) || !plan.layers[(size_t)n_layers - 1].packed) return SICN_EINVAL;
    const RaggedBoundary &b = plan.bounds[(size_t)n_layers], &bi = plan.bounds[(size_t)n_layers - 1];
    cuts->resize((size_t)n_images);
    origins->resize(2 * (size_t)n_images);
    if (live) live->assign((size_t)n_images, 0);
    int64_t off = 0;
    for (int i = 0; i < n_images; i++) {
        const sicn_ragged_rect r = rects ? rects[i] : sicn_ragged_rect{0, 0, b.W[(size_t)i], b.H[(size_t)i]};
        if (r.w < 1 || r.h < 1 || r.x0 < 0 || r.y0 < 0) return SICN_EINVAL;
        if ((int64_t)r.x0 + r.w > b.W[(size_t)i] || (int64_t)r.y0 + r.h > b.H[(size_t)i]) return SICN_EINVAL;
        (*cuts)[(size_t)i] = PlanarOut{r.w, r.h, off};
        (*origins)[2 * (size_t)i] = r.x0;
        (*origins)[2 * (size_t)i + 1] = r.y0;
        off += (int64_t)r.h * r.w * 3;
        if (live) {
            // the test is a product of a row test and a column test: count the rows in the tile column that holds x0 (live in x
            // by construction) and the columns in the tile row that holds y0
            const int cx = r.x0 / RECT_TILE_OUT * ANY_T, cy = r.y0 / RECT_TILE_OUT * ANY_T;
            int64_t ny = 0, nx = 0;
            for (int ty = 0; ty < bi.H[(size_t)i]; ty += ANY_T) ny += rect_tile_live(ty, cx, r.x0, r.y0, r.w, r.h);
            for (int tx = 0; tx < bi.W[(size_t)i]; tx += ANY_T) nx += rect_tile_live(cy, tx, r.x0, r.y0, r.w, r.h);
            (*live)[(size_t)i] = ny * nx;
        }
    }
    *bytes = off;
    return SICN_OK;
}

template <bool DECONV, int NT>
static hipError_t launch_ragged_as(const uint8_t *in, uint8_t *out, const int8_t *wimg, const int8_t *bias, const RaggedRow *rows,
                                   const uint32_t *tile_image, int cin, int cout, unsigned items, uint32_t floor2, hipStream_t stream)
{
    const size_t lds = any_lds_bytes(DECONV);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)k_any_ragged<DECONV, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_any_ragged<DECONV, NT>), dim3(items, (unsigned)((cout + 63) / 64), 1), dim3(256), lds, stream, in, out, wimg, bias,
                       rows, tile_image, cin, cout, floor2);
    return hipGetLastError();
}

}  // namespace sicn

using namespace sicn;

struct sicn_ragged_net {
    int n_layers = 0, n_images = 0;
    RaggedPlan plan;
    std::vector<sicn_layer_desc> descs;
    std::vector<const sicn_weights *> weights;
    std::vector<const sicn_gdn *> gdn;      // per layer: the activation in place of the ReLU, or nullptr
    std::vector<const int8_t *> wimg;       // per layer: the weights' own pack_any image, or one of `owned`
    std::vector<DeviceTable<int8_t>> owned; // images packed here: for weights whose family is another one (the reference's widths), and
                                            // the packed-K images of the RGB ends (ragged_rgb_host.hpp)
    DeviceTable<RaggedRow> d_rows;          // [n_layers][n_images]
    DeviceTable<uint32_t> d_tile_image;     // the layers' tile -> image maps back to back
    std::vector<size_t> map_at;             // per layer: its first entry in d_tile_image
    size_t slot = 0;                        // bytes of one ping-pong buffer
    bool planar_in = false, planar_out = false;   // include/sicn_ragged_planar.h: the pixel layout of boundary -1 and of boundary n - 1
    int64_t out_bytes = 0;                  // bytes of boundary n - 1 as this net lays it out
    DeviceTable<PlanarOut> d_cuts;          // planar or rectangle out: [n_images] the sizes and offsets of the output
    bool rect_out = false;                  // include/sicn_ragged_rect.h: the last layer stores a rectangle of every reconstruction
    DeviceTable<int32_t> d_origins;         // rectangle out: [n_images][2] the creation's origins (x0, y0)
};

extern "C" int sicn_ragged_layout(const sicn_layer_desc *descs, int n_layers, const int32_t *widths, const int32_t *heights, int n_images,
                                  int layer, int image, int64_t out[8])
{
    if (!out) return SICN_EINVAL;
    RaggedPlan p;
    if (int rc = ragged_plan(descs, n_layers, widths, heights, n_images, SICN_RAGGED_RGB_GENERIC, &p)) return rc;
    if (layer < -1 || layer >= n_layers || image < 0 || image >= n_images) return SICN_EINVAL;
    const RaggedBoundary &b = p.bounds[(size_t)(layer + 1)];
    out[0] = b.W[(size_t)image];
    out[1] = b.H[(size_t)image];
    out[2] = b.C;
    out[3] = b.off[(size_t)image];
    out[4] = b.off[(size_t)n_images];
    out[5] = out[6] = out[7] = 0;
    if (layer >= 0) {
        const RaggedLayerPlan &lp = p.layers[(size_t)layer];
        out[5] = lp.first_item[(size_t)image];
        out[6] = lp.tiles_x[(size_t)image];
        out[7] = lp.first_item[(size_t)n_images];
    }
    return SICN_OK;
}

extern "C" void sicn_ragged_net_free(sicn_ragged_net *net) { delete net; }

extern "C" int sicn_ragged_net_create(const sicn_layer_desc *descs, sicn_weights *const *weights, int n_layers, const int32_t *widths,
                                      const int32_t *heights, int n_images, sicn_ragged_net **out)
{
    return sicn_ragged_net_create_gdn(descs, weights, nullptr, n_layers, widths, heights, n_images, out);
}

extern "C" int sicn_ragged_net_create_gdn(const sicn_layer_desc *descs, sicn_weights *const *weights, const sicn_gdn *const *gdn, int n_layers,
                                          const int32_t *widths, const int32_t *heights, int n_images, sicn_ragged_net **out)
{
    return sicn_ragged_net_create_rgb(descs, weights, gdn, n_layers, widths, heights, n_images, SICN_RAGGED_RGB_PACKED, out);
}

extern "C" int sicn_ragged_rgb_layout(const sicn_layer_desc *descs, int n_layers, const int32_t *widths, const int32_t *heights, int n_images,
                                      int rgb_ends, int layer, int image, int64_t out[3])
{
    if (!out) return SICN_EINVAL;
    RaggedPlan p;
    if (int rc = ragged_plan(descs, n_layers, widths, heights, n_images, rgb_ends, &p)) return rc;
    if (layer < 0 || layer >= n_layers || image < 0 || image >= n_images) return SICN_EINVAL;
    const RaggedLayerPlan &lp = p.layers[(size_t)layer];
    out[0] = lp.first_item[(size_t)image];
    out[1] = lp.tiles_x[(size_t)image];
    out[2] = lp.first_item[(size_t)n_images];
    return SICN_OK;
}

extern "C" const char *sicn_ragged_net_kernel_for(const sicn_ragged_net *net, int layer)
{
    if (!net || layer < 0 || layer >= net->n_layers) return nullptr;
    const bool tr = net->descs[(size_t)layer].transposed == 1;
    if (layer == 0 && net->planar_in) return "mfma_conv_rgb_planar";
    if (layer == net->n_layers - 1 && net->rect_out) return net->planar_out ? "mfma_deconv_rgb_planar_rect" : "mfma_deconv_rgb_rect";
    if (layer == net->n_layers - 1 && net->planar_out) return "mfma_deconv_rgb_planar";
    if (net->plan.layers[(size_t)layer].packed) return tr ? "mfma_deconv_rgb_packed" : "mfma_conv_rgb_packed";
    return tr ? "mfma_deconv_any" : "mfma_conv_any";
}

extern "C" int sicn_ragged_net_create_rgb(const sicn_layer_desc *descs, sicn_weights *const *weights, const sicn_gdn *const *gdn, int n_layers,
                                          const int32_t *widths, const int32_t *heights, int n_images, int rgb_ends, sicn_ragged_net **out)
{
    return sicn_ragged_net_create_planar(descs, weights, gdn, n_layers, widths, heights, n_images, rgb_ends, SICN_RAGGED_PIXELS_INTERLEAVED,
                                         SICN_RAGGED_PIXELS_INTERLEAVED, nullptr, nullptr, out);
}

extern "C" int sicn_ragged_planar_layout(const sicn_layer_desc *descs, int n_layers, const int32_t *widths, const int32_t *heights,
                                         int n_images, int pixels_out, const int32_t *out_widths, const int32_t *out_heights, int image,
                                         int64_t out[6])
{
    if (!out) return SICN_EINVAL;
    RaggedPlan p;
    if (int rc = ragged_plan(descs, n_layers, widths, heights, n_images, SICN_RAGGED_RGB_PACKED, &p)) return rc;
    std::vector<PlanarOut> cuts;
    int64_t bytes = 0;
    try {
        if (int rc = planar_out_plan(p, descs, n_layers, n_images, pixels_out, out_widths, out_heights, &cuts, &bytes)) return rc;
    } catch (const std::bad_alloc &) { return SICN_ENOMEM; }
    if (image < 0 || image >= n_images) return SICN_EINVAL;
    out[0] = cuts[(size_t)image].w;
    out[1] = cuts[(size_t)image].h;
    out[2] = cuts[(size_t)image].off;
    out[3] = bytes;
    out[4] = p.bounds[0].off[(size_t)image];
    out[5] = p.bounds[0].off[(size_t)n_images];
    return SICN_OK;
}

// every creation ends here: out_widths / out_heights as sicn_ragged_net_create_planar takes them, or rects as
// sicn_ragged_net_create_rect does (then without sizes)
static int create_net(const sicn_layer_desc *descs, sicn_weights *const *weights, const sicn_gdn *const *gdn, int n_layers,
                      const int32_t *widths, const int32_t *heights, int n_images, int rgb_ends, int pixels_in, int pixels_out,
                      const int32_t *out_widths, const int32_t *out_heights, const sicn_ragged_rect *rects, sicn_ragged_net **out);

extern "C" int sicn_ragged_net_create_planar(const sicn_layer_desc *descs, sicn_weights *const *weights, const sicn_gdn *const *gdn,
                                             int n_layers, const int32_t *widths, const int32_t *heights, int n_images, int rgb_ends,
                                             int pixels_in, int pixels_out, const int32_t *out_widths, const int32_t *out_heights,
                                             sicn_ragged_net **out)
{
    return create_net(descs, weights, gdn, n_layers, widths, heights, n_images, rgb_ends, pixels_in, pixels_out, out_widths, out_heights,
                      nullptr, out);
}

extern "C" int sicn_ragged_net_create_rect(const sicn_layer_desc *descs, sicn_weights *const *weights, const sicn_gdn *const *gdn,
                                           int n_layers, const int32_t *widths, const int32_t *heights, int n_images, int rgb_ends,
                                           int pixels_in, int pixels_out, const sicn_ragged_rect *rects, sicn_ragged_net **out)
{
    return create_net(descs, weights, gdn, n_layers, widths, heights, n_images, rgb_ends, pixels_in, pixels_out, nullptr, nullptr, rects, out);
}

extern "C" int sicn_ragged_rect_layout(const sicn_layer_desc *descs, int n_layers, const int32_t *widths, const int32_t *heights,
                                       int n_images, const sicn_ragged_rect *rects, int image, int64_t out[5])
{
    if (!out) return SICN_EINVAL;
    RaggedPlan p;
    if (int rc = ragged_plan(descs, n_layers, widths, heights, n_images, SICN_RAGGED_RGB_PACKED, &p)) return rc;
    std::vector<PlanarOut> cuts;
    std::vector<int32_t> origins;
    std::vector<int64_t> live;
    int64_t bytes = 0;
    try {
        if (int rc = rect_out_plan(p, descs, n_layers, n_images, SICN_RAGGED_PIXELS_INTERLEAVED, rects, &cuts, &origins, &bytes, &live))
            return rc;
    } catch (const std::bad_alloc &) { return SICN_ENOMEM; }
    if (image < 0 || image >= n_images) return SICN_EINVAL;
    out[0] = cuts[(size_t)image].w;
    out[1] = cuts[(size_t)image].h;
    out[2] = cuts[(size_t)image].off;
    out[3] = bytes;
    out[4] = live[(size_t)image];
    return SICN_OK;
}

static int create_net(const sicn_layer_desc *descs, sicn_weights *const *weights, const sicn_gdn *const *gdn, int n_layers,
                      const int32_t *widths, const int32_t *heights, int n_images, int rgb_ends, int pixels_in, int pixels_out,
                      const int32_t *out_widths, const int32_t *out_heights, const sicn_ragged_rect *rects, sicn_ragged_net **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    if (!weights) return SICN_EINVAL;
    return make_object(out, [&](sicn_ragged_net &net) {
        if (int rc = ragged_plan(descs, n_layers, widths, heights, n_images, rgb_ends, &net.plan)) return rc;
        // the pixel layouts: a planar end is the packed-K kernel of that end with another loader or epilogue, nothing else
        if (pixels_in != SICN_RAGGED_PIXELS_INTERLEAVED && pixels_in != SICN_RAGGED_PIXELS_PLANAR) return SICN_EINVAL;
        net.planar_in = pixels_in == SICN_RAGGED_PIXELS_PLANAR;
        std::vector<PlanarOut> cuts;
        if (int rc = planar_out_plan(net.plan, descs, n_layers, n_images, pixels_out, out_widths, out_heights, &cuts, &net.out_bytes)) return rc;
        net.planar_out = pixels_out == SICN_RAGGED_PIXELS_PLANAR;
        // rectangles: the same table with the rectangles' sizes, and the origins beside it
        std::vector<int32_t> origins;
        if (rects) {
            if (rgb_ends != SICN_RAGGED_RGB_PACKED || (gdn && gdn[n_layers - 1])) return SICN_EINVAL;
            if (int rc = rect_out_plan(net.plan, descs, n_layers, n_images, pixels_out, rects, &cuts, &origins, &net.out_bytes, nullptr)) return rc;
            net.rect_out = true;
        }
        if ((net.planar_in || net.planar_out) && rgb_ends != SICN_RAGGED_RGB_PACKED) return SICN_EINVAL;
        if (net.planar_in && !(descs[0].transposed == 0 && descs[0].IFM_CH == 3)) return SICN_EINVAL;
        if (net.planar_out && gdn && gdn[n_layers - 1]) return SICN_EINVAL;
        for (int l = 0; l < n_layers; l++) {
            const sicn_weights *w = weights[l];
            if (!w || w->cin != descs[l].IFM_CH || w->cout != descs[l].OFM_CH || w->transposed != descs[l].transposed) return SICN_EINVAL;
            if (gdn && gdn[l] && gdn[l]->channels != descs[l].OFM_CH) return SICN_EINVAL;
        }
        if (int rc = chip_geom(nullptr)) return rc;       // no device, or not a gfx950 one
        net.n_layers = n_layers;
        net.n_images = n_images;
        net.descs.assign(descs, descs + n_layers);
        net.weights.assign(weights, weights + n_layers);
        net.gdn.assign((size_t)n_layers, nullptr);
        if (gdn) net.gdn.assign(gdn, gdn + n_layers);
        // the tables: one row per (layer, image), one tile -> image entry per tile
        std::vector<RaggedRow> rows((size_t)n_layers * n_images);
        ItemMap map;
        size_t mx = 0;
        for (int l = 0; l < n_layers; l++) {
            const RaggedBoundary &bi = net.plan.bounds[(size_t)l], &bo = net.plan.bounds[(size_t)l + 1];
            const RaggedLayerPlan &lp = net.plan.layers[(size_t)l];
            const int per_tile = lp.per_tile;
            net.map_at.push_back(map.size());
            for (int i = 0; i < n_images; i++) {
                rows[(size_t)l * n_images + i] = RaggedRow{bi.W[(size_t)i], bi.H[(size_t)i], bo.W[(size_t)i], bo.H[(size_t)i], lp.tiles_x[(size_t)i],
                                                           (int32_t)lp.first_item[(size_t)i], bi.off[(size_t)i], bo.off[(size_t)i]};
                map.add((size_t)((lp.first_item[(size_t)i + 1] - lp.first_item[(size_t)i]) / per_tile), (uint32_t)i);
            }
            if (l + 1 < n_layers && (size_t)bo.off[(size_t)n_images] > mx) mx = (size_t)bo.off[(size_t)n_images];
        }
        net.slot = (mx + 255) / 256 * 256;
        if (!net.d_rows.upload(rows) || !map.upload(net.d_tile_image)) return SICN_ENOMEM;
        if ((net.planar_out || net.rect_out) && !net.d_cuts.upload(cuts)) return SICN_ENOMEM;
        if (net.rect_out && !net.d_origins.upload(origins)) return SICN_ENOMEM;
        // the weight image: weights of a width the specialised families serve were uploaded without one (sicn_weights_from_finn_tiles
        // packs the images of the family the shape runs on); pack it here from the plain [cout][25 cin] copy every handle has
        for (int l = 0; l < n_layers; l++) {
            const sicn_weights *w = weights[l];
            const bool packed = net.plan.layers[(size_t)l].packed;
            if (!packed && w->d_w_any) {
                net.wimg.push_back(w->d_w_any);
                continue;
            }
            const size_t img_bytes = !packed ? any_bytes(w->cin, w->cout) : w->transposed ? rgb_deconv_bytes(w->cin) : rgb_conv_bytes(w->cout);
            std::vector<int8_t> okc((size_t)w->cout * 25 * w->cin), img(img_bytes);
            if (hipMemcpy(okc.data(), w->d_w_okc, okc.size(), hipMemcpyDeviceToHost) != hipSuccess) return SICN_ENODEV;
            if (!packed)
                pack_any(okc.data(), w->cin, w->cout, img.data());
            else if (w->transposed)
                pack_rgb_deconv(okc.data(), w->cin, img.data());
            else
                pack_rgb_conv(okc.data(), w->cout, img.data());
            DeviceTable<int8_t> dev;
            if (!dev.upload(img)) return SICN_ENOMEM;
            net.wimg.push_back(dev.get());
            net.owned.push_back(std::move(dev));
        }
        return SICN_OK;
    });
}

extern "C" size_t sicn_ragged_net_workspace_bytes(const sicn_ragged_net *net) { return net ? 2 * net->slot : 0; }

extern "C" int sicn_ragged_net_forward(const sicn_ragged_net *net, int first, int last, const uint8_t *in, uint8_t *out, int tap_layer,
                                       uint8_t *tap_out, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    return sicn_ragged_net_forward_at(net, first, last, in, out, tap_layer, tap_out, workspace, workspace_bytes, nullptr, hip_stream);
}

extern "C" int sicn_ragged_net_forward_at(const sicn_ragged_net *net, int first, int last, const uint8_t *in, uint8_t *out, int tap_layer,
                                          uint8_t *tap_out, void *workspace, size_t workspace_bytes, const int32_t *origins_dev,
                                          void *hip_stream)
{
    if (!net || !in || !out) return SICN_EINVAL;
    if (origins_dev && (!net->rect_out || last != net->n_layers - 1 || ((uintptr_t)origins_dev & 3u))) return SICN_EINVAL;
    if (first < 0 || last >= net->n_layers || first > last) return SICN_EINVAL;
    if (tap_layer >= 0 && (tap_layer < first || tap_layer > last || !tap_out)) return SICN_EINVAL;
    if (last > first && (!workspace || workspace_bytes < 2 * net->slot)) return SICN_ENOSPC;
    if (int rc = chip_geom(nullptr)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *pp[2] = {(uint8_t *)workspace, (uint8_t *)workspace + net->slot};
    const uint8_t *cur = in;
    for (int l = first; l <= last; l++) {
        // a tapped layer is written straight into the caller's buffer and the next layer reads it there, as in sicn_net_forward
        uint8_t *dst = (l == last) ? out : (l == tap_layer ? tap_out : pp[(l - first) & 1]);
        const sicn_layer_desc &d = net->descs[(size_t)l];
        const sicn_weights *w = net->weights[(size_t)l];
        const RaggedRow *rows = net->d_rows.get() + (size_t)l * net->n_images;
        const uint32_t *map = net->d_tile_image.get() + net->map_at[(size_t)l];
        const unsigned items = (unsigned)net->plan.layers[(size_t)l].first_item[(size_t)net->n_images];
        const int8_t *wimg = net->wimg[(size_t)l];
        const sicn_gdn *g = net->gdn[(size_t)l];
        const uint32_t floor2 = g ? ACT_FLOOR_RAW : ACT_FLOOR_RELU;
        const bool planar_out = net->planar_out && l == net->n_layers - 1, rect_out = net->rect_out && l == net->n_layers - 1;
        const size_t in_bytes = (size_t)net->plan.bounds[(size_t)l].off[(size_t)net->n_images];
        const size_t out_bytes = planar_out || rect_out ? (size_t)net->out_bytes : (size_t)net->plan.bounds[(size_t)l + 1].off[(size_t)net->n_images];
        hipError_t e;
        if (net->planar_in && l == 0)
            e = launch_ragged_rgb_conv_planar(cur, in_bytes, dst, wimg, w->d_bias, rows, map, d.OFM_CH, items, floor2, stream);
        else if (rect_out)
            e = launch_ragged_rgb_deconv_rect(planar_out, cur, dst, wimg, w->d_bias, rows, map, net->d_cuts.get(),
                                              origins_dev ? origins_dev : net->d_origins.get(), d.IFM_CH, items, floor2, stream);
        else if (planar_out)
            e = launch_ragged_rgb_deconv_planar(cur, dst, wimg, w->d_bias, rows, map, net->d_cuts.get(), d.IFM_CH, items, floor2, stream);
        else if (net->plan.layers[(size_t)l].packed)
            e = d.transposed ? launch_ragged_rgb_deconv(cur, dst, wimg, w->d_bias, rows, map, d.IFM_CH, items, floor2, stream)
                             : launch_ragged_rgb_conv(cur, in_bytes, dst, wimg, w->d_bias, rows, map, d.OFM_CH, items, floor2, stream);
        else if (d.transposed)
            e = d.OFM_CH == 3 ? launch_ragged_as<true, 1>(cur, dst, wimg, w->d_bias, rows, map, d.IFM_CH, d.OFM_CH, items, floor2, stream)
                              : launch_ragged_as<true, 4>(cur, dst, wimg, w->d_bias, rows, map, d.IFM_CH, d.OFM_CH, items, floor2, stream);
        else
            e = launch_ragged_as<false, 4>(cur, dst, wimg, w->d_bias, rows, map, d.IFM_CH, d.OFM_CH, items, floor2, stream);
        if (e != hipSuccess) return SICN_ENODEV;
        // the activation, in place wherever the layer wrote: the ragged tensor is [positions of all images][OFM_CH]
        if (g)
            if (int rc = gdn_apply_lanes(*g, dst, (long long)(out_bytes / (size_t)d.OFM_CH), stream)) return rc;
        if (l == tap_layer && tap_out != dst) {
            if (hipMemcpyAsync(tap_out, dst, out_bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess) return SICN_ENODEV;
        }
        cur = dst;
    }
    return SICN_OK;
}

// ---- ragged crop: dst image i = the top-left [dst_h][dst_w][C] of src image i --------------------------------------------------------
// The cut (k_ragged_window.hip) of the rectangles (0, 0, dst_w, dst_h) without source offsets; a crop handle IS a cut handle.
static sicn_ragged_cut *as_cut(sicn_ragged_crop *crop) { return reinterpret_cast<sicn_ragged_cut *>(crop); }
static const sicn_ragged_cut *as_cut(const sicn_ragged_crop *crop) { return reinterpret_cast<const sicn_ragged_cut *>(crop); }
static sicn_ragged_crop *as_crop(sicn_ragged_cut *cut) { return reinterpret_cast<sicn_ragged_crop *>(cut); }

// the arguments are checked before dst_w and dst_h are read; what an image may be is the cut's to say
static int corner_rects(const int32_t *src_w, const int32_t *src_h, const int32_t *dst_w, const int32_t *dst_h, int channels, int n_images,
                        std::vector<sicn_ragged_rect> *rects)
{
    if (!src_w || !src_h || !dst_w || !dst_h || n_images < 1 || channels < 1) return SICN_EINVAL;
    try {
        rects->resize((size_t)n_images);
    } catch (const std::bad_alloc &) { return SICN_ENOMEM; }
    for (int i = 0; i < n_images; i++) (*rects)[(size_t)i] = sicn_ragged_rect{0, 0, dst_w[i], dst_h[i]};
    return SICN_OK;
}

extern "C" int sicn_ragged_crop_layout(const int32_t *src_w, const int32_t *src_h, const int32_t *dst_w, const int32_t *dst_h, int channels,
                                       int n_images, int image, int64_t out[4])
{
    if (!out) return SICN_EINVAL;
    std::vector<sicn_ragged_rect> rects;
    if (int rc = corner_rects(src_w, src_h, dst_w, dst_h, channels, n_images, &rects)) return rc;
    return ragged_cut_layout(src_w, src_h, rects.data(), channels, nullptr, n_images, image, out);
}

extern "C" int sicn_ragged_crop_create(const int32_t *src_w, const int32_t *src_h, const int32_t *dst_w, const int32_t *dst_h, int channels,
                                       int n_images, sicn_ragged_crop **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    std::vector<sicn_ragged_rect> rects;
    if (int rc = corner_rects(src_w, src_h, dst_w, dst_h, channels, n_images, &rects)) return rc;
    sicn_ragged_cut *cut = nullptr;
    const int rc = ragged_cut_create(src_w, src_h, rects.data(), channels, nullptr, n_images, &cut);
    *out = as_crop(cut);
    return rc;
}

extern "C" void sicn_ragged_crop_free(sicn_ragged_crop *crop) { sicn_ragged_cut_free(as_cut(crop)); }

extern "C" int sicn_ragged_crop_run(const sicn_ragged_crop *crop, const uint8_t *src, uint8_t *dst, void *hip_stream)
{
    return ragged_cut_run(as_cut(crop), src, dst, hip_stream);
}
