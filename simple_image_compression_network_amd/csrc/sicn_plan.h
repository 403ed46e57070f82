// Launch planning: every number a launcher derives from the SIZE OF THE CHIP lives here, as pure host functions of a
// ChipGeom (compute units, XCDs) — nothing in csrc/ hard-wires 256 CUs / 8 XCDs any more.  chip_geom() reads the current
// device's hipDeviceProp_t once per device (sicn_abi.hip); the functions below are what tests/test_abi_load.py walks for
// 256, 128 and 32 CUs through sicn_debug_plan (no GPU needed).
//
// The rule (include/sicn.h, "Device"): the device must be a gfx950 part (gcnArchName starts with "gfx950"), else every entry
// point that would touch it returns SICN_ENODEV.  n_cu = multiProcessorCount.  n_xcd = the largest power of two <= 8 with at
// least 20 CUs per XCD (MI355X SPX: 256 CUs -> 8 XCDs of 32; DPX 128 -> 4; QPX 64 -> 2; CPX 32 -> 1; a part with fused-off CUs,
// e.g. 240, keeps its 8).  hipDeviceProp_t has no XCD count; the mapping only steers which tiles share an L2, never results.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sicn {

struct ChipGeom {
    int n_cu;    // compute units of the device (partition) the stream runs on
    int n_xcd;   // XCDs = L2 domains; workgroups of a 1-D grid are dealt to them round-robin
};

inline int xcd_count_for(int n_cu)
{
    int n = 8;
    while (n > 1 && n_cu / n < 20) n >>= 1;
    return n;
}
inline ChipGeom chip_from_cus(int n_cu) { return ChipGeom{n_cu < 1 ? 1 : n_cu, xcd_count_for(n_cu)}; }

// XCD-aware work list (k_common.hpp xcd_logical_index is the device side): grids are padded to a multiple of n_xcd
inline unsigned xcd_grid_size(long n_items, int n_xcd) { return (unsigned)((n_items + n_xcd - 1) / n_xcd * n_xcd); }
// host mirror of the device mapping: logical item of workgroup `block`, or -1
inline long xcd_item_of(long block, long n_items, int n_xcd)
{
    const long per = (n_items + n_xcd - 1) / n_xcd;
    const long idx = (block % n_xcd) * per + block / n_xcd;
    return (block / n_xcd < per && idx < n_items) ? idx : -1;
}

// ---- the wide persistent kernels (k_mfma16x.hip): one resident workgroup per CU ---------------------------------------------
constexpr int WIDE_MIN_TILES_PER_CU = 4;
// workgroups of a wide launch: one per CU, at most one per tile, a multiple of n_xcd; grid_cap > 0 (tests) lowers it
inline unsigned wide_grid(long total_tiles, int grid_cap, const ChipGeom &c)
{
    long cap = c.n_cu / c.n_xcd * c.n_xcd;
    if (cap < c.n_xcd) cap = c.n_xcd;
    if (grid_cap > 0) {
        cap = (long)grid_cap / c.n_xcd * c.n_xcd;
        if (cap < c.n_xcd) cap = c.n_xcd;
    }
    const long need = (total_tiles + c.n_xcd - 1) / c.n_xcd * c.n_xcd;
    return (unsigned)(need < cap ? need : cap);
}
// the dynamic part of the wide kernels' tile deal (k_mfma16x.hip DealX: one ticket counter per XCD + one mailbox per workgroup in the call's
// workspace).  It pays where a workgroup walks many tiles (measured r05 on 256 CUs: 32 tiles each in layers 1 / 6 of 8 x 4K, - 13 and - 9 us);
// with 8 (layers 2 / 5) one tile is 12 % of a workgroup's work, nothing can be balanced and the look at the other XCDs' counters at the end
// only costs (+ 3 us): static there
constexpr int WIDE_DEAL_MAX_XCDS = 16, WIDE_DEAL_MAX_WORKGROUPS = 512, WIDE_DEAL_MIN_TILES_PER_WORKGROUP = 16;
inline bool wide_deal_pays(long total_tiles, unsigned grid, const ChipGeom &c)
{
    return grid <= (unsigned)WIDE_DEAL_MAX_WORKGROUPS && c.n_xcd <= WIDE_DEAL_MAX_XCDS && total_tiles >= (long)WIDE_DEAL_MIN_TILES_PER_WORKGROUP * grid;
}
// automatic choice of the wide form: from WIDE_MIN_TILES_PER_CU tiles (16 x 32) per CU on; the conv already from 3.5 rounds
// when the last round is at least 90 % full (measured r03 on 256 CUs: 1020 tiles 131 - 140 us against 144 - 149)
inline bool wide_automatic(long tiles_w, bool deconv, const ChipGeom &c)
{
    const long n = c.n_cu;
    const long rounds = (tiles_w + n - 1) / n;
    const bool full_rounds = tiles_w * 10 >= rounds * n * 9;
    return tiles_w >= n * WIDE_MIN_TILES_PER_CU || (!deconv && full_rounds && 2 * tiles_w >= 7 * n);
}

// ---- the 8 x 16 / 8 x 32 kernels (k_mfma16.hip, k_mfma16p.hip): two resident workgroups per CU ----------------------------
// 8 x 32 tiles from about 0.8 of one residency on (measured r03 on 256 CUs: the bar sat at 416 - 434 of 512 tiles)
inline bool narrow_tile_wanted(long tiles32, const ChipGeom &c) { return tiles32 * 16 < 13L * 2 * c.n_cu; }
// output-channel split of the 8 x 16 kernels: grids that leave half of the CUs without a workgroup (measured r02: <= 128 of 256)
inline bool split_n_automatic(long tiles16, const ChipGeom &c) { return tiles16 * 2 <= c.n_cu; }

// ---- the channel-generic kernels (k_mfma16c.hip): 16 x 16 M positions x 64 output channels per workgroup ---------------------
// grid x = tiles (x 4 phases for the deconv, the phase in the low two bits so that the four workgroups of a tile run together and
// share its input lines), y = blocks of 64 output channels, z = images.  The served form has one tile size and no persistent grid,
// so nothing here depends on the chip.  grid_x == 0: the layer does not fit a launch.
struct AnyPlan { int tile, tiles_x, tiles_y; unsigned grid_x, grid_y, grid_z; };
inline AnyPlan plan_any(int m_w, int m_h, int cout, int deconv, int n_images)
{
    AnyPlan p{16, (m_w + 15) / 16, (m_h + 15) / 16, 0u, (unsigned)((cout + 63) / 64), (unsigned)n_images};
    const long long gx = (long long)p.tiles_x * p.tiles_y * (deconv ? 4 : 1);
    if (gx > 0 && gx < 0x7fffffffLL && n_images > 0 && n_images <= 65535) p.grid_x = (unsigned)gx;
    return p;
}

// ---- the RGB layers (k_rgb.hip, k_l0g.hip): vertical strips of TILE_X columns, each cut into runs ---------------------------------
// The tile sizes are here, once, for the kernels and for the planning; the launchers and sicn_debug_plan call the same functions.
constexpr int TILE_X = 32;     // columns of a strip (and of an M tile of the 8 x 32 implicit-GEMM kernels, sicn_internal.h)
constexpr int L0_TY = 8;       // layer 0: output rows per tile (wave w = rows 2w, 2w+1)
constexpr int L0_CHUNK = 9;    // layer 0: tiles a workgroup walks at most (its raw pixels are LDS-resident)
constexpr int L0G_CHUNK = 8;   // the same for layer 0 fused with its GDN (8 is the most two workgroups' LDS holds)
constexpr int L7_ROWS = 4;     // layer 7: input rows per step

// layer 7: y_chunks runs per strip, just under TWO workgroups per CU in all (measured r03: 510 of 512 best); every cut re-fetches
// six halo rows and the weights.  forced > 0 (sicn_options.strip_chunks): that many runs.  A 1-D XCD-aware grid.
struct L7Plan { int tiles_x, steps_y, y_chunks; unsigned grid_x; };
inline L7Plan plan_l7(int iw, int ih, int n_images, int forced, const ChipGeom &c)
{
    L7Plan p{(iw + TILE_X - 1) / TILE_X, (ih + L7_ROWS - 1) / L7_ROWS, 0, 0u};
    long y = forced > 0 ? forced : (2L * c.n_cu) / ((long)p.tiles_x * n_images);
    if (y < 1) y = 1;
    if (y > p.steps_y) y = p.steps_y;
    p.y_chunks = (int)y;
    p.grid_x = xcd_grid_size((long)p.tiles_x * p.y_chunks * n_images, c.n_xcd);
    return p;
}

// layer 0: vertical runs of at most L0_CHUNK (fused with a GDN: L0G_CHUNK) tiles per workgroup, evened out; about four workgroups
// per CU on small images; forced > 0 can only shorten the runs.  Grid = tiles_x x y_chunks x n_images.
struct L0Plan { int tiles_x, tiles_y, y_chunks, ty_per; };
inline L0Plan plan_l0(int ow, int oh, int n_images, bool gdn_fused, int forced, const ChipGeom &c)
{
    const int tiles_x = (ow + TILE_X - 1) / TILE_X, tiles_y = (oh + L0_TY - 1) / L0_TY, max_run = gdn_fused ? L0G_CHUNK : L0_CHUNK;
    int y_chunks = (tiles_y + max_run - 1) / max_run;
    long want = (4L * c.n_cu + (long)tiles_x * n_images - 1) / ((long)tiles_x * n_images);
    if (forced > 0) want = forced;
    if (want > y_chunks) y_chunks = want > tiles_y ? tiles_y : (int)want;
    const int ty_per = (tiles_y + y_chunks - 1) / y_chunks;
    return L0Plan{tiles_x, tiles_y, (tiles_y + ty_per - 1) / ty_per, ty_per};
}

}  // namespace sicn
