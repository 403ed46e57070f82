// Ragged nets, the RGB ends in their packed-K form (include/sicn_ragged_rgb.h): conv 3 -> N and deconv N -> 3 over n images of n
// different sizes, one launch per layer.  The tile bodies are rgb_conv_tile() / rgb_deconv_tile() (k_rgb_ragged_body.hpp), functions
// of one image; the kernels here only resolve item -> image from the tables of k_ragged.hip (tile_image, RaggedRow), with
// wave-uniform loads pinned to scalar registers, as k_any_ragged does.
//
// Grid: x = the layer's work items over all images.  Conv: one 16 x 16 tile of output positions, the same cut and the same
// first_item as the channel-generic form; y = 1 — the blocks of 64 output channels are a loop inside the workgroup (the kernel
// strides them by gridDim.y), so the patch and its expansion are paid once per tile.  Deconv: one 16 x 16 tile of input positions
// with all four phases: tile_image is indexed by the item itself and first_item is the per-tile cut's.
//
// k_rgb_conv_ragged_planar and k_rgb_deconv_ragged_planar (include/sicn_ragged_planar.h) are the same two kernels at a planar
// boundary: the same grids and tables, the conv with planar_quad as its loader, the deconv with the cut epilogue.
//
// k_rgb_deconv_ragged_rect<PLANAR> (include/sicn_ragged_rect.h) is the deconv with the rectangle epilogue in either layout: the sizes
// and offsets from a PlanarOut table, the origins from an int32 [n_images][2] array that may be the caller's.  A workgroup whose
// tile does not meet its image's rectangle returns before it loads anything else.
#include "k_ragged_common.hpp"
#include "k_rgb_ragged_body.hpp"

namespace sicn {

struct RaggedItem {
    int IW, IH, OW, OH, ty, tx;
    uint64_t in_off, out_off;
};

__device__ __forceinline__ RaggedItem ragged_item(const RaggedRow *__restrict__ rows, const uint32_t *__restrict__ tile_image)
{
    const int item = (int)blockIdx.x;
    const RaggedRow *row = rows + uni(tile_image[item]);
    RaggedItem r;
    r.IW = (int)uni((uint32_t)row->IW);
    r.IH = (int)uni((uint32_t)row->IH);
    r.OW = (int)uni((uint32_t)row->OW);
    r.OH = (int)uni((uint32_t)row->OH);
    const int tiles_x = (int)uni((uint32_t)row->tiles_x);
    const int local = item - (int)uni((uint32_t)row->first_item);
    r.in_off = uni((uint64_t)row->in_off);
    r.out_off = uni((uint64_t)row->out_off);
    r.ty = local / tiles_x;
    r.tx = local - r.ty * tiles_x;
    return r;
}

__global__ __launch_bounds__(256) void k_rgb_conv_ragged(const uint8_t *__restrict__ in, uint64_t in_bytes, uint8_t *__restrict__ out,
                                                         const int8_t *__restrict__ wimg, const int8_t *__restrict__ bias,
                                                         const RaggedRow *__restrict__ rows, const uint32_t *__restrict__ tile_image, int O,
                                                         uint32_t floor2)
{
    __shared__ __attribute__((aligned(16))) uint8_t smem[RGBC_LDS];
    const RaggedItem r = ragged_item(rows, tile_image);
    rgb_conv_tile(in + r.in_off, in, in + in_bytes, out + r.out_off, wimg, bias, r.IW, r.IH, r.OW, r.OH, O, r.ty * ANY_T, r.tx * ANY_T,
                  (int)blockIdx.y, (int)gridDim.y, floor2, smem);
}

__global__ __launch_bounds__(256) void k_rgb_deconv_ragged(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                           const int8_t *__restrict__ wimg, const int8_t *__restrict__ bias,
                                                           const RaggedRow *__restrict__ rows, const uint32_t *__restrict__ tile_image, int C,
                                                           uint32_t floor2)
{
    __shared__ __attribute__((aligned(16))) uint8_t smem[RGBD_LDS];
    const RaggedItem r = ragged_item(rows, tile_image);
    rgb_deconv_tile<false>(in + r.in_off, out + r.out_off, wimg, bias, r.IW, r.IH, C, r.OW, r.OH, r.ty * ANY_T, r.tx * ANY_T, floor2, smem);
}

// The planar siblings (include/sicn_ragged_planar.h): `in` holds the images as [3][IH][IW] planes at the same offsets, `out` as
// [3][h][w] planes cut to the sizes and placed at the offsets of `cuts` — a table of its own, RaggedRow keeps its layout.
__global__ __launch_bounds__(256) void k_rgb_conv_ragged_planar(const uint8_t *__restrict__ in, uint64_t in_bytes, uint8_t *__restrict__ out,
                                                                const int8_t *__restrict__ wimg, const int8_t *__restrict__ bias,
                                                                const RaggedRow *__restrict__ rows, const uint32_t *__restrict__ tile_image,
                                                                int O, uint32_t floor2)
{
    __shared__ __attribute__((aligned(16))) uint8_t smem[RGBC_LDS];
    const RaggedItem r = ragged_item(rows, tile_image);
    rgb_conv_tile_planar(in + r.in_off, in, in + in_bytes, out + r.out_off, wimg, bias, r.IW, r.IH, r.OW, r.OH, O, r.ty * ANY_T,
                         r.tx * ANY_T, (int)blockIdx.y, (int)gridDim.y, floor2, smem);
}

__global__ __launch_bounds__(256) void k_rgb_deconv_ragged_planar(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                                  const int8_t *__restrict__ wimg, const int8_t *__restrict__ bias,
                                                                  const RaggedRow *__restrict__ rows, const uint32_t *__restrict__ tile_image,
                                                                  const PlanarOut *__restrict__ cuts, int C, uint32_t floor2)
{
    __shared__ __attribute__((aligned(16))) uint8_t smem[RGBD_LDS];
    const RaggedItem r = ragged_item(rows, tile_image);
    const PlanarOut *cut = cuts + uni(tile_image[(int)blockIdx.x]);
    const int w = (int)uni((uint32_t)cut->w), h = (int)uni((uint32_t)cut->h);
    rgb_deconv_tile<true>(in + r.in_off, out + uni((uint64_t)cut->off), wimg, bias, r.IW, r.IH, C, w, h, r.ty * ANY_T, r.tx * ANY_T, floor2,
                          smem);
}

// The rectangle forms: `out` holds image i as [h][w][3] (PLANAR: [3][h][w]) at cuts[i].off, the rectangle (origins[2 i],
// origins[2 i + 1], cuts[i].w, cuts[i].h) of its reconstruction.  The grid is the layer's fixed one; the tile test depends on
// blockIdx alone, so the whole workgroup returns together, before the first load of the patch and before the first __syncthreads().
template <bool PLANAR>
__device__ __forceinline__ void rgb_deconv_ragged_rect(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const int8_t *__restrict__ wimg,
                                                       const int8_t *__restrict__ bias, const RaggedRow *__restrict__ rows,
                                                       const uint32_t *__restrict__ tile_image, const PlanarOut *__restrict__ cuts,
                                                       const int32_t *__restrict__ origins, int C, uint32_t floor2, uint8_t *smem)
{
    const RaggedItem r = ragged_item(rows, tile_image);
    const uint32_t img = uni(tile_image[(int)blockIdx.x]);
    const PlanarOut *cut = cuts + img;
    const int w = (int)uni((uint32_t)cut->w), h = (int)uni((uint32_t)cut->h);
    const int32_t rx0 = (int32_t)uni((uint32_t)origins[2 * (size_t)img]), ry0 = (int32_t)uni((uint32_t)origins[2 * (size_t)img + 1]);
    if (!rect_tile_live(r.ty * ANY_T, r.tx * ANY_T, rx0, ry0, w, h)) return;
    rgb_deconv_tile<PLANAR, true>(in + r.in_off, out + uni((uint64_t)cut->off), wimg, bias, r.IW, r.IH, C, w, h, r.ty * ANY_T, r.tx * ANY_T,
                                  floor2, smem, rx0, ry0);
}

__global__ __launch_bounds__(256) void k_rgb_deconv_ragged_rect(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                                const int8_t *__restrict__ wimg, const int8_t *__restrict__ bias,
                                                                const RaggedRow *__restrict__ rows, const uint32_t *__restrict__ tile_image,
                                                                const PlanarOut *__restrict__ cuts, const int32_t *__restrict__ origins,
                                                                int C, uint32_t floor2)
{
    __shared__ __attribute__((aligned(16))) uint8_t smem[RGBD_LDS];
    rgb_deconv_ragged_rect<false>(in, out, wimg, bias, rows, tile_image, cuts, origins, C, floor2, smem);
}

__global__ __launch_bounds__(256) void k_rgb_deconv_ragged_planar_rect(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                                       const int8_t *__restrict__ wimg, const int8_t *__restrict__ bias,
                                                                       const RaggedRow *__restrict__ rows,
                                                                       const uint32_t *__restrict__ tile_image,
                                                                       const PlanarOut *__restrict__ cuts, const int32_t *__restrict__ origins,
                                                                       int C, uint32_t floor2)
{
    __shared__ __attribute__((aligned(16))) uint8_t smem[RGBD_LDS];
    rgb_deconv_ragged_rect<true>(in, out, wimg, bias, rows, tile_image, cuts, origins, C, floor2, smem);
}

bool ragged_rgb_packed_serves(int cin, int cout, int transposed)
{
    if (!any_supported(cin, cout, transposed)) return false;
    return transposed ? cout == 3 : cin == 3;
}

hipError_t launch_ragged_rgb_conv(const uint8_t *in, size_t in_bytes, uint8_t *out, const int8_t *wimg, const int8_t *bias,
                                  const RaggedRow *rows, const uint32_t *tile_image, int cout, unsigned items, uint32_t floor2,
                                  hipStream_t stream)
{
    hipLaunchKernelGGL(k_rgb_conv_ragged, dim3(items, 1, 1), dim3(256), 0, stream, in, (uint64_t)in_bytes, out, wimg, bias, rows, tile_image,
                       cout, floor2);
    return hipGetLastError();
}

hipError_t launch_ragged_rgb_deconv(const uint8_t *in, uint8_t *out, const int8_t *wimg, const int8_t *bias, const RaggedRow *rows,
                                    const uint32_t *tile_image, int cin, unsigned items, uint32_t floor2, hipStream_t stream)
{
    hipLaunchKernelGGL(k_rgb_deconv_ragged, dim3(items, 1, 1), dim3(256), 0, stream, in, out, wimg, bias, rows, tile_image, cin, floor2);
    return hipGetLastError();
}

hipError_t launch_ragged_rgb_conv_planar(const uint8_t *in, size_t in_bytes, uint8_t *out, const int8_t *wimg, const int8_t *bias,
                                         const RaggedRow *rows, const uint32_t *tile_image, int cout, unsigned items, uint32_t floor2,
                                         hipStream_t stream)
{
    hipLaunchKernelGGL(k_rgb_conv_ragged_planar, dim3(items, 1, 1), dim3(256), 0, stream, in, (uint64_t)in_bytes, out, wimg, bias, rows,
                       tile_image, cout, floor2);
    return hipGetLastError();
}

hipError_t launch_ragged_rgb_deconv_planar(const uint8_t *in, uint8_t *out, const int8_t *wimg, const int8_t *bias, const RaggedRow *rows,
                                           const uint32_t *tile_image, const PlanarOut *cuts, int cin, unsigned items, uint32_t floor2,
                                           hipStream_t stream)
{
    hipLaunchKernelGGL(k_rgb_deconv_ragged_planar, dim3(items, 1, 1), dim3(256), 0, stream, in, out, wimg, bias, rows, tile_image, cuts, cin,
                       floor2);
    return hipGetLastError();
}

hipError_t launch_ragged_rgb_deconv_rect(bool planar, const uint8_t *in, uint8_t *out, const int8_t *wimg, const int8_t *bias,
                                         const RaggedRow *rows, const uint32_t *tile_image, const PlanarOut *cuts, const int32_t *origins,
                                         int cin, unsigned items, uint32_t floor2, hipStream_t stream)
{
    if (planar)
        hipLaunchKernelGGL(k_rgb_deconv_ragged_planar_rect, dim3(items, 1, 1), dim3(256), 0, stream, in, out, wimg, bias, rows, tile_image,
                           cuts, origins, cin, floor2);
    else
        hipLaunchKernelGGL(k_rgb_deconv_ragged_rect, dim3(items, 1, 1), dim3(256), 0, stream, in, out, wimg, bias, rows, tile_image, cuts,
                           origins, cin, floor2);
    return hipGetLastError();
}

}  // namespace sicn
