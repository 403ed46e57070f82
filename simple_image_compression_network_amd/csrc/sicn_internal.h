// Internal declarations shared by the libsicn.so translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/sicn.h"
#include "sicn_plan.h"

namespace sicn {

// Geometry of the implicit-GEMM kernels (k_mfma16*.hip).  One workgroup owns an "M tile" of
// TILE_Y x TILE_X positions of the M grid (conv: output pixels; deconv: input pixels) and all
// output channels.  LDS holds sub-patches of (TILE_Y+2) x (TILE_X+2) positions x 32 bytes.
constexpr int TILE_Y = 8;                      // TILE_X = 32: sicn_plan.h
constexpr int PATCH_Y = TILE_Y + 2;
constexpr int KSTEP = 32;                      // bytes of K per MFMA (v_mfma_i32_32x32x32_i8)

enum KernelKind : int { KK_GENERIC = 0, KK_MFMA_CONV, KK_MFMA_DECONV, KK_L0_RGB, KK_L7_RGB, KK_MFMA_CONV_ANY, KK_MFMA_DECONV_ANY };

struct LayerGeom {
    int IW, IH, CIN, OW, OH, COUT, transposed;
};

inline LayerGeom geom_of(const sicn_layer_desc &d)
{
    return LayerGeom{d.IFM_ROW, d.IFM_COL, d.IFM_CH, d.OFM_ROW, d.OFM_COL, d.OFM_CH, d.transposed};
}

}  // namespace sicn

struct sicn_ragged_coder;   // k_ragged_codec.hip
struct sicn_ragged_ctx_coder;   // k_ragged_ctx.hip
struct sicn_ragged_cut;     // k_ragged_window.hip
struct sicn_ragged_rect;    // include/sicn_ragged_window.h

// One layer's device-resident parameters, in every layout a kernel family wants.
struct sicn_weights {
    int cin, cout, transposed;
    int8_t *d_w_okc;      // [cout][25*cin] int8, k = (ky*5+kx)*cin + c        (generic kernel)
    int8_t *d_bias;       // [cout] int8
    int8_t *d_w_mfma16;    // implicit-GEMM tile stream for v_mfma_i32_16x16x64_i8 (k_mfma16.hip), or nullptr when the shape is not served by it
    int8_t *d_w_mfma16x;   // deconv 128 -> 128: the tiles in the order the wide persistent kernel walks them (k_mfma16x.hip), or nullptr
    // layer-0 (RGB -> cout) and layer-7 (cin -> RGB) layouts, or nullptr
    int8_t *d_w_l0;
    int8_t *d_w_l0g;       // layer 0, 128 channels: the A-operand image of the kernel that applies a GDN before its store (k_l0g.hip)
    int8_t *d_w_l7;
    int8_t *d_w_l7_half;   // layer 7: the 6 KB image of the kernel form that reads the channels 0 .. 63 only (k_rgb.hip: pack_l7_half)
    int8_t *d_w_any;       // the channel-generic MFMA kernels' weight image (k_mfma16c.hip: pack_any), or nullptr when they do not serve the shape
    // what d_w_okc and d_bias were uploaded from: a net's live-channel plan (sicn_live.h) reads them and derives permuted images
    std::vector<int8_t> h_w_okc, h_bias;
};

namespace sicn {

// the tile deal of the wide persistent kernels: 16 ticket counters (one per XCD) + one mailbox per workgroup
constexpr int DEAL_MAX_WORKGROUPS = WIDE_DEAL_MAX_WORKGROUPS;
constexpr int DEAL_WORDS = WIDE_DEAL_MAX_XCDS + DEAL_MAX_WORKGROUPS;
hipError_t launch_zero_words(unsigned long long *p, size_t words, hipStream_t stream);   // k_generic.hip

// what plan_mfma (k_mfma16.hip) decides for a conv / deconv layer of the 128 / 192-channel shapes
struct MfmaPlan {
    int family;      // 1: the software-pipelined kernels (k_mfma16p.hip), 2: the wide persistent kernels (k_mfma16x.hip)
    int tile_x;      // 16 | 32 (family 1)
    int split_n;     // output-channel slices (workgroups of blockIdx.y), 1 = none
    unsigned grid_x, grid_y, grid_z;
    int deal;        // family 2: 1 where the tile deal has its dynamic part (sicn_plan.h wide_deal_pays), given a workspace with room for it
};
MfmaPlan plan_mfma(const LayerGeom &g, int n_images, const sicn_options &o, const ChipGeom &chip);
// library defaults: zeros overridden by the SICN_* environment as it was at load time (read once)
const sicn_options &default_options();
// experiment switches, read once at load.  no_deal (SICN_NO_DEAL=1): the static tile deal even with a workspace (A/B)
struct DebugEnv { int no_deal; };
const DebugEnv &debug_env();

// Geometry of the CURRENT device (hipGetDevice), read once per device from hipDeviceProp_t: SICN_OK, or SICN_ENODEV when there
// is no device or it is not a gfx950 part (the code objects of this library exist for gfx950 only)
int chip_geom(ChipGeom *out);

// Launchers: enqueue on `stream`, return hipError_t of the launch.  `chip`: sizes every grid (sicn_plan.h).
// relu = false: store the lane BEFORE the sign-bit ReLU (input of the GDN extension, include/sicn_gdn.h)
hipError_t launch_generic(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out,
                          int n_images, hipStream_t stream, bool relu = true);
// k_generic.hip: dst[n][h][w][c] = the top-left h x w corner of src[n][hs][ws][c], one launch
hipError_t launch_crop_nhwc(const uint8_t *src, uint8_t *dst, int n, int hs, int ws, int h, int w, int c, hipStream_t stream);
// in_layout / out_layout: LAYOUT_NHWC (the ABI layout) / LAYOUT_GROUP / LAYOUT_PHASE (k_common.hpp)
// deal: DEAL_WORDS zeroed words for the wide persistent kernels' tile deal (k_mfma16x.hip: DealX), or nullptr (static deal)
hipError_t launch_mfma16(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out,
                         int n_images, hipStream_t stream, int in_layout, int out_layout, const sicn_options &o, const ChipGeom &chip,
                         bool relu = true, unsigned long long *deal = nullptr, int columns = 8, int walk_groups = 4);
// k_mfma16x.hip: the wide persistent form — one workgroup of 4 waves per CU walks through 16 x 32-position tiles, 128 x 128 outputs
// per wave (accumulators in AGPRs, one wave per SIMD); grid_cap > 0 limits the number of workgroups (tests)
bool wide_supported(const LayerGeom &g);
size_t mfma16x_deconv_stream_bytes(int cin, int cout);   // 0 where the wide deconv does not exist
void pack_mfma16x_deconv_stream(const int8_t *w_okc, int cin, int cout, int8_t *dst);
hipError_t launch_wide(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out, int n_images, hipStream_t stream,
                       int in_layout, int out_layout, bool relu, int grid_cap, const ChipGeom &chip, unsigned long long *deal = nullptr,
                       int columns = 8, int walk_groups = 4);   // walk_groups: sicn_live.h — only a net's call plan ever says 3
// k_mfma16x_live.hip: the same kernels with the first `columns` (3 | 5) of the 8 accumulator columns only, for weights permuted by the
// net's live-channel plan (sicn_live.h); nullptr for a width that is not built
const void *wide_live_kernel(int transposed, bool nt_store, int columns);
// k_mfma16x_g3.hip: the conv with the three-group K walk, `columns` 3 | 5 | 8; nullptr for a width that is not built
const void *wide_g3_kernel(bool nt_store, int columns);
// k_mfma16p.hip: the software-pipelined conv / deconv kernels (tile_x = 16 | 32)
bool pipelined_supported(const LayerGeom &g, int tile_x);
hipError_t launch_pipelined(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out, int n_images,
                            hipStream_t stream, int in_layout, int out_layout, bool relu, int tile_x, bool split_channels,
                            const ChipGeom &chip);
// groups = 3: the kernel computes and stores the 32-channel groups 0 .. 2 only (out_layout GROUP: plane 3 stays what it held); the
// caller knows that the weight rows 96 .. 127 of `w` belong to channels nobody reads (sicn_live.h)
hipError_t launch_l0(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out,
                     int n_images, hipStream_t stream, int out_layout, const sicn_options &o, const ChipGeom &chip, bool relu = true,
                     int groups = 4);
hipError_t launch_l7(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out,
                     int n_images, hipStream_t stream, int in_layout, const sicn_options &o, const ChipGeom &chip, int halves = 2);

// Host-side weight packers (pure CPU, unit-testable without a GPU).
// w_okc: [cout][25*cin].  Returns bytes written into `dst` (size from *_bytes()).
bool mfma_supported(int cin, int cout, int transposed);
size_t mfma16_stream_bytes(int cin, int cout);
void pack_mfma16_stream(const int8_t *w_okc, int cin, int cout, int transposed, int8_t *dst);

// k_mfma16c.hip: conv2d<> / deconv522<> at any served channel width (run-time channel counts), NHWC in and out
bool any_supported(int cin, int cout, int transposed);
size_t any_bytes(int cin, int cout);
void pack_any(const int8_t *w_okc, int cin, int cout, int8_t *dst);
hipError_t launch_any(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out, int n_images, hipStream_t stream,
                      bool relu = true);

// k_ragged_rgb.hip: the packed-K kernels of a ragged net's RGB ends (include/sicn_ragged_rgb.h) — conv 3 -> N, deconv N -> 3; the
// tables are k_ragged.hip's (RaggedRow: k_ragged_common.hpp), the weight images pack_rgb_conv / pack_rgb_deconv's (ragged_rgb_host.hpp)
struct RaggedRow;
bool ragged_rgb_packed_serves(int cin, int cout, int transposed);
hipError_t launch_ragged_rgb_conv(const uint8_t *in, size_t in_bytes, uint8_t *out, const int8_t *wimg, const int8_t *bias,
                                  const RaggedRow *rows, const uint32_t *tile_image, int cout, unsigned items, uint32_t floor2,
                                  hipStream_t stream);
hipError_t launch_ragged_rgb_deconv(const uint8_t *in, uint8_t *out, const int8_t *wimg, const int8_t *bias, const RaggedRow *rows,
                                    const uint32_t *tile_image, int cin, unsigned items, uint32_t floor2, hipStream_t stream);
// their planar siblings (include/sicn_ragged_planar.h): `in` as [3][IH][IW] planes; `out` as [3][h][w] planes at the sizes and
// offsets of `cuts` (PlanarOut: ragged_planar_host.hpp), one entry per image
struct PlanarOut;
hipError_t launch_ragged_rgb_conv_planar(const uint8_t *in, size_t in_bytes, uint8_t *out, const int8_t *wimg, const int8_t *bias,
                                         const RaggedRow *rows, const uint32_t *tile_image, int cout, unsigned items, uint32_t floor2,
                                         hipStream_t stream);
hipError_t launch_ragged_rgb_deconv_planar(const uint8_t *in, uint8_t *out, const int8_t *wimg, const int8_t *bias, const RaggedRow *rows,
                                           const uint32_t *tile_image, const PlanarOut *cuts, int cin, unsigned items, uint32_t floor2,
                                           hipStream_t stream);

// k_ragged_codec.hip: a ragged coder as the window decoder (k_ragged_window.hip) sees it — [n_images] CoderRow (k_codec_body.hpp)
// on the host and on the device, both owned by the coder
struct RaggedCoderView {
    int n_images;
    const void *rows_host, *d_rows;
    size_t row_bytes;
    uint64_t ws_bytes;
};
void ragged_coder_view(const sicn_ragged_coder *coder, RaggedCoderView *v);
// k_ragged_ctx.hip: the same of a ragged ctx coder as the moving ROI decode (k_ragged_ctx_roi_move.hip) sees it — [n_images] CtxRow
// (k_ctx_body.hpp); host only
void ragged_ctx_coder_view(const sicn_ragged_ctx_coder *coder, RaggedCoderView *v);

// k_ragged_window.hip: the one rectangle copy of the ragged family, behind sicn_ragged_cut_* (sicn_ragged_window.h) as they stand and
// behind sicn_ragged_crop_* (sicn_ragged_hyper.h, k_ragged.hip) as the cut at the corner.  Arguments and codes: sicn_ragged_cut_*
int ragged_cut_layout(const int32_t *src_w, const int32_t *src_h, const sicn_ragged_rect *rects, int channels,
                      const uint64_t *src_offset_or_null, int n_images, int image, int64_t out[4]);
int ragged_cut_create(const int32_t *src_w, const int32_t *src_h, const sicn_ragged_rect *rects, int channels,
                      const uint64_t *src_offset_or_null, int n_images, sicn_ragged_cut **out);
int ragged_cut_run(const sicn_ragged_cut *cut, const uint8_t *src, uint8_t *dst, void *hip_stream);
// the same kernel over tables that are not a sicn_ragged_cut's own (k_ragged_roi_move.hip writes its rows on the stream): d_rows is
// [images] sicn_window::CutRow, d_item_image [items], both in device memory.  Enqueue only; SICN_OK or SICN_ENODEV
int ragged_cut_launch(const void *d_rows, const uint32_t *d_item_image, unsigned items, const uint8_t *src, uint8_t *dst, void *hip_stream);

size_t l0_bytes(int cout);
void pack_l0(const int8_t *w_okc, int cout, int8_t *dst);
size_t l0g_bytes();
void pack_l0g(const int8_t *w_okc, int8_t *dst);   // cout = 128
size_t l7_bytes(int cin);
void pack_l7(const int8_t *w_okc, int cin, int8_t *dst);
size_t l7_half_bytes();
void pack_l7_half(const int8_t *w_okc, int8_t *dst);   // cin = 128

}  // namespace sicn
