// conv2d<> / deconv522<> with 128 / 192 channels on v_mfma_i32_16x16x64_i8: which kernels a layer runs with (plan_mfma), the
// launch (launch_mfma16) and the host-side packing of the weight stream the kernels walk.  The kernels themselves live in
// k_mfma16p.hip (software-pipelined 8 x 16 / 8 x 32 tiles: decomposition, lane roles and C/D layout are described there) and
// k_mfma16x.hip (the wide persistent form of the 128 -> 128 layers).
#include "k_common.hpp"

namespace sicn {

// Which kernel family, tile width and splits a conv / deconv layer runs with (pure: sicn_debug_plan walks it without a GPU).
//   family 2: the wide persistent form (k_mfma16x.hip: one workgroup of 4 waves per CU, 16 x 32 positions, 128 x 128 outputs per
//             wave) where every CU gets at least WIDE_MIN_TILES_PER_CU tiles; sicn_options.wave_tile = 128 forces it, 64 forbids it
//   family 1: the software-pipelined 8 x 16 / 8 x 32 kernels (k_mfma16p.hip) everywhere else
// Tile width: 8 x 32 positions by default; 8 x 16 for the 192-channel layers (the only width their kernels exist at: the wide tile
// would allow one workgroup per CU) and where the wide tile leaves most of the chip without a tile (small images).
// sicn_options.tile_x = 16 | 32 forces one where both exist (experiments, tests).
MfmaPlan plan_mfma(const LayerGeom &g, int n_images, const sicn_options &o, const ChipGeom &chip)
{
    const bool deconv = g.transposed != 0;
    const int nt16 = g.COUT / 16;
    const int MW = deconv ? g.IW : g.OW, MH = deconv ? g.IH : g.OH;
    MfmaPlan p{1, 32, 1, 0, 1, 1, 0};
    if (wide_supported(g) && o.tile_x != 16) {
        const long tiles_w = (long)((MW + 31) / 32) * ((MH + 15) / 16) * n_images;
        // measured r03 (tools/ab_options.py, 1080p x 4 and 4K x 1 = 1020 tiles of 256 CUs): layer 1 131 - 140 against 144 - 149 us;
        // at 255 / 510 tiles the wide conv loses, 44 / 39 and 70 / 68 us; the deconv is a wash below 1024: 45 / 47, 75 / 75, 146 / 142 us
        if (o.wave_tile == 128 || (o.wave_tile == 0 && o.prefetch == 0 && wide_automatic(tiles_w, deconv, chip))) {
            p.family = 2;
            p.grid_x = wide_grid(tiles_w, o.persistent_grid, chip);
            p.deal = wide_deal_pays(tiles_w, p.grid_x, chip);
            return p;
        }
    }
    const long tiles32 = (long)((MW + 31) / 32) * ((MH + TILE_Y - 1) / TILE_Y) * n_images;
    // 8 x 32 tiles from about 0.8 of one residency (2 workgroups per CU) on: below that the 8 x 16 tiles' second, partly filled
    // round is still cheaper; measured r03 on one image of 1440 x 810 ... 1920 x 1080 (312 ... 506 tiles of 8 x 32), layer 1 / 6:
    // 8 x 16 tiles 30 31 | 38 39 39 / 39 40 | 47 47 46 us, 8 x 32 tiles 35 35 | 35 36 36 / 40 40 | 41 42 41 us (the bar at 434 tiles)
    const bool wide_tile = pipelined_supported(g, 32);
    bool narrow = !wide_tile || narrow_tile_wanted(tiles32, chip);
    if (o.tile_x == 16) narrow = true;
    if (o.tile_x == 32 && wide_tile) narrow = false;
    p.tile_x = narrow ? 16 : 32;
    const long tiles = (long)((MW + p.tile_x - 1) / p.tile_x) * ((MH + TILE_Y - 1) / TILE_Y) * n_images;
    p.grid_x = xcd_grid_size(tiles, chip.n_xcd);
    // grids that leave half of the CUs without a workgroup: split the output channels over 2 / 3 workgroups
    // (measured, r02: at 192 - 255 tiles the split is a wash or a loss; at <= 72 it takes 20 - 35 % off the layer)
    if (p.tile_x == 16 && (o.split_n > 1 || (o.split_n == 0 && split_n_automatic(tiles, chip)))) p.split_n = nt16 / 4;
    p.grid_y = p.split_n;
    return p;
}

// shapes the 16x16x64 kernels serve: the reference net's L1-L6 plus the hyperprior stacks' conv 192 -> 128 and deconv 128 -> 192
bool mfma_supported(int cin, int cout, int transposed)
{
    (void)transposed;
    return (cin == 128 || cin == 192) && (cout == 128 || cout == 192) && !(cin == 192 && cout == 192);
}

hipError_t launch_mfma16(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out, int n_images,
                         hipStream_t stream, int in_layout, int out_layout, const sicn_options &o, const ChipGeom &chip, bool relu,
                         unsigned long long *deal, int columns, int walk_groups)
{
    if ((size_t)g.IH * g.IW * g.CIN >= (size_t)OOB) return hipErrorInvalidValue;          // 31-bit patch offsets
    if ((size_t)g.OH * g.OW * g.COUT >= (size_t)OOB) return hipErrorInvalidValue;         // buffer-descriptor stores
    if (!mfma_supported(g.CIN, g.COUT, g.transposed)) return hipErrorInvalidValue;
    const MfmaPlan p = plan_mfma(g, n_images, o, chip);
    if (p.family == 2) return launch_wide(g, w, in, out, n_images, stream, in_layout, out_layout, relu, o.persistent_grid, chip, deal, columns,
                                          walk_groups);
    if (columns != 8) return hipErrorInvalidValue;   // only the wide family skips columns (sicn_live.h)
    // (round 2 sent the deconv 192 -> 128 on full grids back to a plain, unpipelined kernel: the pipelined one was 7 % slower there.
    // The reason was the v_mov copies hipcc made for its run-time buffer parity — right around the asm MFMAs, where
    // tools/isa_hazards.py found them; with the parity static the pipelined form is 17 % FASTER: layer 4 0.158 -> 0.131 ms.)
    return launch_pipelined(g, w, in, out, n_images, stream, in_layout, out_layout, relu, p.tile_x, p.split_n > 1, chip);
}

// ---- host-side weight packing: the tile sequence of the 32x32x32 form, rows in the 16x16 C/D
// ---- order (LDS row j*16 + rho holds channel 64*(j>>2) + 16*(rho>>2) + 4*(j&3) + (rho&3)), no swizzle;
// ---- PAD16 zero tiles behind the stream (k_common.hpp).  The tile packer and the conv's group-major order: conv_walk.hpp
size_t mfma16_stream_bytes(int cin, int cout) { return (size_t)(25 * (cin / 32) + PAD16) * cout * KSTEP; }

void pack_mfma16_stream(const int8_t *w_okc, int cin, int cout, int transposed, int8_t *dst)
{
    const int nq = cin / 32;
    const size_t tb = (size_t)cout * KSTEP;
    size_t step = 0;
    if (!transposed) {
        pack_conv_stream16(w_okc, cin, cout, dst);
        step = (size_t)25 * nq;
    } else {
        for (int ph = 0; ph < 4; ph++) {
            const int py = ph >> 1, px = ph & 1;
            for (int iy = 0; iy < 3 - py; iy++)
                for (int ix = 0; ix < 3 - px; ix++) {
                    const int ky = 2 * iy + py, kx = 2 * ix + px;
                    for (int q = 0; q < nq; q++) pack_tile16(w_okc, cin, cout, ky * 5 + kx, q, dst + (step++) * tb);
                }
        }
    }
    for (size_t i = step * tb; i < (step + PAD16) * tb; i++) dst[i] = 0;
}

}  // namespace sicn
