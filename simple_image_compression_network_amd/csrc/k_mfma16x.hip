// conv2d<> / deconv522<> 128 -> 128 (layers 1, 2 / 5, 6: 70 % of the step) — the WIDE PERSISTENT form (round 3).
//
// Where k_mfma16p.hip stands: 2 workgroups x 4 waves per CU, 64 positions x 128 channels per wave, 12 fragment
// reads per 32 MFMAs, every workgroup streams its own copy of the weights; the passes are issue-bound and a bare loop of that
// structure tops out at 3.44 POP/s (tools/microbench/wide_dma.hip, profiles/r03_microbench_wide_dma.txt).  The same
// microbenchmark says what the alternative keeps once it carries a real pass's load: ONE wave per SIMD with 128 positions x 128
// channels per wave (256 accumulators pinned in registers, 16 fragment reads per 64 MFMAs), 4 LDS-DMA requests, a counted wait and a
// workgroup barrier per pass: 3.75 POP/s, +9 %.  Round 2's k_conv128w had that tile but lost it all in its per-tile prologue and
// epilogue, which nothing covers when a SIMD holds a single wave.  Here
//   * one workgroup of 4 waves per CU owns 16 x 32 positions (wave w = rows 4w .. 4w+3) and is PERSISTENT: it walks through its
//     share of the tile list, the input of the next tile arrives under the current one, the weight stream wraps: no prologue;
//   * the ACCUMULATOR HAND-OVER (read, bias, ReLU, pack, store of a finished tile / deconv phase) is woven into the first pass
//     of the next one: that pass's MFMAs take C = bias and overwrite an accumulator right after it has been read out (in-kernel
//     stamps: done as a block between two tiles the hand-over was 6350 cycles = 10 % of a conv tile, with a single wave per SIMD
//     every VALU instruction costs 4 issue cycles).  The bias is that pass's C operand, so it costs no instruction at all;
//   * the REGISTER FILES of k_deconv_x (four hand-overs per tile): the two operand-fragment sets pa / wa / pb / wb (32 x 4 = 128
//     registers) live in AGPRs — nothing but ds_read_b128 ("=a") writes them and nothing but an MFMA's SrcA / SrcB ("a") reads them,
//     both of which gfx950 takes from either file — and that frees the VGPRs for the accumulators, which the hand-over's pack
//     (VALU: VGPR sources only) then reads in place.  Accumulator columns j >= JV and their bias sit in VGPRs (C and D of an MFMA
//     share a file), columns j < JV in AGPRs:
//         k_deconv_x  JV = 2, fragments in AGPRs:  255 VGPRs, 200 AGPRs (128 fragments + 2 x 36)
//         k_conv_x    JV = 7, fragments in VGPRs:  225 VGPRs, 252 AGPRs (one hand-over per tile: with JV = 3 and the fragments in
//                     AGPRs — 256 + 232 registers, no scratch — layers 1 / 2 measured the same to 0.1 %, so it keeps this map)
//     Per hand-over (64 accumulator tiles, counted in this file's ISA): 256 v_max_i32_sdwa (the pack: one per register, the
//     minimum) + v_accvgpr_read_b32: 64 (deconv), 224 (conv; the deconv's number too until its fragments moved); 16 stores.  No
//     scratch, no VGPR spill, 38 / 40 spilled SGPRs (tests/test_wide_regfile_build.py holds all of that, and each kernel's
//     fragment register file, to the shipped ISA);
//   * the tile list is dealt STATICALLY (XCD x works through the contiguous range [x * per, (x + 1) * per) of the list, its 32
//     workgroups interleaved): with one workgroup per CU all tiles take the same time, so there is no scheduler state at all;
//   * one weight ring per CU (not two): half the weight requests per MFMA; a 16 x 32 tile has 10 % less halo than two 8 x 32;
//   * every LDS read is an asm statement with an immediate offset (no address arithmetic in the loop) and hand-placed waits, the
//     MFMAs are asm statements with the accumulator tied to its register ("+a" / "+v"): the order written is the order issued;
//   * the ring has 10 slots = 5 passes: a 50-pass tile is 0 mod 5, so every slot and every offset of the unrolled tile is a
//     compile-time constant, and 3 passes' requests may be in flight at a barrier.
// Conv:   4 parity planes of one channel group (18 x 34 positions x 32 B, 20 KiB each) with a rolling refresh + ring = 120 KB.
// Deconv: the 18 x 34 patch with all 4 channel groups, as 2 group PAIRS in 3 rotating 40-KiB buffers (the next tile's first pair
//         lands in the spare buffer, its second pair in the buffer the current tile's last phase frees first) + ring = 160 KB.
// Hazards hipcc cannot see inside asm are covered by hand and CHECKED: tools/isa_hazards.py runs over this file's ISA in build().
// The templates (passes, hand-over, tile deal, the two kernel bodies) live in k_mfma16x_body.hpp and take the number of accumulator
// columns NJ; this file instantiates all 8 of them, k_mfma16x_live.hip the 3- and 5-column kernels of a net's live-channel plan.
#include "k_mfma16x_body.hpp"

namespace sicn {
namespace xw {

// all 8 accumulator columns: what every 128 -> 128 layer runs unless the net's live-channel plan (sicn_live.h) finds columns that
// nobody reads — those launches go to k_mfma16x_live.hip
template <bool NT, int JV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_conv_x(SICN_WIDE_KERNEL_ARGS)
{
    conv_x_body<NT, JV, 8, 4>(SICN_WIDE_KERNEL_PASS);
}
template <bool NT, int JV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_deconv_x(SICN_WIDE_KERNEL_ARGS)
{
    deconv_x_body<NT, JV, 8>(SICN_WIDE_KERNEL_PASS);
}

}  // namespace xw

// ---- host side --------------------------------------------------------------------------------------------------------------
// the deconv's weight stream in the order k_deconv_x walks it (dpass): tile 2 T + h = (tap of pass T, channel group 2 pair + h),
// rows as in pack_mfma16_stream
size_t mfma16x_deconv_stream_bytes(int cin, int cout) { return (cin == 128 && cout == 128) ? (size_t)2 * xw::NPASS * cout * KSTEP : 0; }
void pack_mfma16x_deconv_stream(const int8_t *w_okc, int cin, int cout, int8_t *dst)
{
    const int kk = 25 * cin;
    const size_t tb = (size_t)cout * KSTEP;
    for (int T = 0; T < xw::NPASS; T++) {
        const xw::DPass p = xw::dpass(T);
        const int ky = 2 * p.iy + (p.phase >> 1), kx = 2 * p.ix + (p.phase & 1);
        for (int hh = 0; hh < 2; hh++) {
            int8_t *tile = dst + (size_t)(2 * T + hh) * tb;
            const int q = 2 * p.pair + hh;
            for (int row = 0; row < cout; row++) {
                const int j = row >> 4, rho = row & 15;
                const int ch = 64 * (j >> 2) + 16 * (rho >> 2) + 4 * (j & 3) + (rho & 3);
                const int8_t *src = w_okc + (size_t)ch * kk + (ky * 5 + kx) * cin + q * 32;
                for (int b = 0; b < 32; b++) tile[row * 32 + b] = src[b];
            }
        }
    }
}

// conv / deconv 128 -> 128 on 16 x 32 tiles by one persistent workgroup per CU
bool wide_supported(const LayerGeom &g) { return g.CIN == 128 && g.COUT == 128; }

// walk_groups = 3: the three-group K walk, which only a net's call plan asks for (sicn_live.h: walk_groups)
hipError_t launch_wide(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out, int n_images, hipStream_t stream,
                       int in_layout, int out_layout, bool relu, int grid_cap, const ChipGeom &chip, unsigned long long *deal, int columns,
                       int walk_groups)
{
    using namespace xw;
    if (!wide_supported(g)) return hipErrorInvalidValue;
    if (g.transposed && !w.d_w_mfma16x) return hipErrorInvalidValue;
    // the three-group walk is the conv's, and three groups are three planes of the GROUP layout
    if (walk_groups == 3 && (g.transposed || in_layout != LAYOUT_GROUP)) return hipErrorInvalidValue;
    if ((size_t)g.IH * g.IW * g.CIN >= (size_t)OOB || (size_t)g.OH * g.OW * g.COUT >= (size_t)OOB) return hipErrorInvalidValue;
    const int MW = g.transposed ? g.IW : g.OW, MH = g.transposed ? g.IH : g.OH;
    const int tiles_x = (MW + TX - 1) / TX, tiles_y = (MH + TY - 1) / TY;
    const long total = (long)tiles_x * tiles_y * n_images;
    if (total <= 0 || total > 0x7fffffffL) return hipErrorInvalidValue;
    const uint32_t flags = relu ? ACT_FLOOR_RELU : ACT_FLOOR_RAW;
    const bool nt = nt_store_wanted((size_t)g.OH * g.OW * g.COUT * n_images);
    const unsigned grid = wide_grid(total, grid_cap, chip);   // one resident per CU, a multiple of the XCD count (sicn_plan.h)
    // columns < 8: the weight image w is permuted so that the channels the next layer reads fill the first `columns` columns
    const void *fn = walk_groups == 3 ? wide_g3_kernel(nt, columns)
                     : columns != 8 ? wide_live_kernel(g.transposed, nt, columns)
                     : g.transposed ? (nt ? (const void *)&k_deconv_x<true, JV_DECONV> : (const void *)&k_deconv_x<false, JV_DECONV>)
                                    : (nt ? (const void *)&k_conv_x<true, JV_CONV> : (const void *)&k_conv_x<false, JV_CONV>);
    if (!fn) return hipErrorInvalidValue;   // a width that is not built: the plan never asks for one
    const size_t lds = g.transposed ? DECONV_LDS : CONV_LDS;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const int8_t *ws = g.transposed ? w.d_w_mfma16x : w.d_w_mfma16;
    int IW = g.IW, IH = g.IH, OW = g.OW, OH = g.OH, n_tiles = tiles_x * tiles_y, txs = tiles_x;
    uint32_t fl = flags;
    int n_xcd = chip.n_xcd;
    static_assert(DEAL_MAILBOX0 == WIDE_DEAL_MAX_XCDS, "the mailboxes start behind the XCDs' counters");
    if (!wide_deal_pays(total, grid, chip)) deal = nullptr;   // few tiles per workgroup: all of them dealt statically (sicn_plan.h)
    void *args[] = {(void *)&in, (void *)&out, (void *)&ws, (void *)&w.d_bias, &IW, &IH, &OW, &OH, &txs, &n_tiles, &n_images, &in_layout, &out_layout, &fl, &n_xcd,
                    (void *)&deal};
    e = hipLaunchKernel(fn, dim3(grid), dim3(256), args, lds, stream);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

}  // namespace sicn
