// The two RGB-facing layers of the net — HBM-bound streaming kernels that still use int8 MFMA so
// the arithmetic stays far below the memory time:
//
//   k_l0 : conv2d<> with IFM_CH = 3 (layer 0, conv_nonsquare_top.cpp:282-286 / 299-301):
//          reads 3 B/pixel, writes OFM_CH B per output pixel (the bound: SURVEY.md §8d).
//   k_l7 : deconv522<> with OFM_CH = 3 (layer 7, conv_nonsquare_top.cpp:351-353):
//          reads IFM_CH B/pixel (the bound), writes 4 x 3 B per input position.
//
// Both follow the closed forms of SURVEY.md §8(a) a8/a9 (bit-exact, wrap mod 256, relu7).
#include <cstdlib>

#include <algorithm>

#include "k_l0_common.hpp"

namespace sicn {

// One workgroup = a vertical run of up to L0_CHUNK tiles of one 32-pixel strip.  The output stores
// of this kernel complete slowly when the chip streams 4-6 TB/s of them, and vmcnt retires in
// order: a wait for ANY load issued after a tile's stores is a wait for those stores (with one wait
// per tile the kernel ran at 4.5 TB/s of stores even without its MFMAs).  So the loop contains no
// load at all: the raw pixels of the whole run (3 B/pixel: 30 KB for 9 tiles), the weights and the
// bias are brought into LDS by one burst of LDS-DMA in the prologue, and per tile the kernel only
// expands the next tile's pixels LDS -> LDS, runs its MFMAs and issues its 8 stores per wave
// (lanes outside the image: out-of-range offset of a buffer descriptor), separated by a raw barrier.
// The two workgroups of a CU cover each other's prologue.
// NTJ = 32-channel groups of the output LAYOUT (COUT = 32 NTJ: the image stride, the weight image, the bias).  NG = groups that are
// computed and stored: NG < NTJ leaves the planes NG .. NTJ - 1 of the GROUP layout as the tensor held them (their channels are dead by
// the net's plan, sicn_live.h; launch_l0 hands such a kernel nothing but the GROUP layout).  The weight image is loaded whole, its rows
// j >= NG are never read; accumulators, MFMAs and stores run over NG groups.  k_l0<4> = k_l0<4, 4> is the kernel it was.
template <int NTJ, int NG = NTJ>
__global__ __launch_bounds__(256, 2) void k_l0(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                               const int8_t *__restrict__ w_l0,
                                               const int8_t *__restrict__ bias, int IW, int IH, int OW,
                                               int OH, int tiles_y, int ty_per, int out_layout, uint32_t act_floor)
{
    static_assert(NG >= 1 && NG <= NTJ, "computed groups of the NTJ groups of the layout");
    constexpr int COUT = NTJ * 32;
    constexpr int TB = COUT * KSTEP;
    constexpr int WBYTES = 5 * TB;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *wl = smem;
    uint8_t *patch0 = smem + WBYTES;                  // two patches of L0_PATCH bytes (16-byte multiples)
    uint8_t *bias_lds = patch0 + 2 * L0_PATCH;
    uint8_t *raw = bias_lds + 128;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 31, kh = lane >> 5;
    const int img = blockIdx.z;
    const int X0 = blockIdx.x * TILE_X;
    const int ty_begin = blockIdx.y * ty_per, ty_end = min(tiles_y, ty_begin + ty_per);   // ty_per <= L0_CHUNK
    if (ty_begin >= ty_end) return;  // before any LDS-DMA is issued

    const int im_bytes = IH * IW * 3;
    const int img_byte0 = img * im_bytes;                       // launch_l0 guarantees the tensor is < 2 GiB
    const int tensor_bytes4 = ((int)gridDim.z * im_bytes + 3) & ~3;
    uint8_t *out_img = out + (size_t)img * OH * OW * COUT;
    const TensorMap om = tensor_map(out_layout, COUT, OW, OH);

    // ---- prologue: everything this workgroup will ever read ------------------------------------
    {
        // raw rows 2*Y - 2 .. of the run, 52 dwords each from the dword holding pixel 2*X0-2: lane l of
        // instruction k fetches dword idx = 64k + l (row idx / 52, dword idx % 52) through a descriptor over
        // the WHOLE input tensor (its base is allocator-aligned, an image base need not be; rows outside the
        // image and offsets outside the tensor read 0)
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)in, 0, tensor_bytes4, 0x00020000);
        const int rows = 2 * L0_TY * (ty_end - ty_begin) + 3;
        const int n_instr = (rows * L0_RAW_DW + 63) / 64;
        for (int k = w; k < n_instr; k += 4) {
            const int idx = 64 * k + lane;
            const int r = idx / L0_RAW_DW, c = idx - r * L0_RAW_DW;
            const int iy = 2 * L0_TY * ty_begin - 2 + r;
            const int o = ((img_byte0 + (iy * IW + 2 * X0 - 2) * 3) & ~3) + 4 * c;   // negative only left of the very first pixel
            const bool ok = r < rows && iy >= 0 && iy < IH && o >= 0;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, LDS_PTR(raw + k * 256), 4, ok ? (uint32_t)o : OOB, 0, 0, 0);
        }
        // weights: 5 tiles of [COUT][32 B] (row permutation + half swizzle as in k_mfma), linear copy
        for (int piece = w; piece < WBYTES / 1024; piece += 4)
            __builtin_amdgcn_global_load_lds(GLB_PTR(w_l0 + piece * 1024 + lane * 16), LDS_PTR(wl + piece * 1024), 16, 0, 0);
        if (tid < COUT / 4) ((uint32_t *)bias_lds)[tid] = ((const uint32_t *)bias)[tid];
    }
    uint32_t wrow[NG];
#pragma unroll
    for (int j = 0; j < NG; j++) wrow[j] = (uint32_t)((j * 32 + m) * 32 + ((kh ^ ((m >> 3) & 1)) << 4));
    // the builtin (not inline asm): hipcc then KNOWS no LDS-DMA is pending and puts no vmcnt(0) of
    // its own in front of the LDS accesses of the loop
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    block_barrier();
    l0_expand(raw, patch0, img_byte0, tid, ty_begin * L0_TY, X0, IW, IH);
    l0_expand(raw, patch0, img_byte0, tid + 256, ty_begin * L0_TY, X0, IW, IH);
    block_barrier();

    int buf = 0;
    for (int tile_y = ty_begin; tile_y < ty_end; tile_y++, buf ^= 1) {
        const int Y0 = tile_y * L0_TY;
        const uint8_t *patch = patch0 + buf * L0_PATCH;
        if (tile_y + 1 < ty_end) {   // pixels of the next tile -> the patch nobody reads in this iteration
            const uint8_t *rsrc = raw + (tile_y + 1 - ty_begin) * (2 * L0_TY * L0_RAW_DW * 4);
            uint8_t *nxt = patch0 + (buf ^ 1) * L0_PATCH;
            l0_expand(rsrc, nxt, img_byte0, tid, Y0 + L0_TY, X0, IW, IH);
            l0_expand(rsrc, nxt, img_byte0, tid + 256, Y0 + L0_TY, X0, IW, IH);
        }

        v16i acc[2][NG];
#pragma unroll
        for (int j = 0; j < NG; j++) {
            const v4i b4 = *(const v4i *)(bias_lds + j * 32 + 16 * kh);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int bv = (int)(int8_t)((uint32_t)b4[r >> 2] >> (8 * (r & 3)));
                acc[0][j][r] = bv;
                acc[1][j][r] = bv;
            }
        }
#pragma unroll
        for (int ky = 0; ky < 5; ky++) {
            v4i wf[NG], pf[2];
#pragma unroll
            for (int j = 0; j < NG; j++) wf[j] = *(const v4i *)(wl + ky * TB + wrow[j]);
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const uint8_t *src = patch + (2 * (2 * w + i) + ky) * L0_PITCH + 8 * m + 16 * kh;
                const uint2 lo = *(const uint2 *)src, hi = *(const uint2 *)(src + 8);
                pf[i] = v4i{(int)lo.x, (int)lo.y, (int)hi.x, (int)hi.y};
            }
#pragma unroll
            for (int j = 0; j < NG; j++)
#pragma unroll
                for (int i = 0; i < 2; i++)
                    acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[j], pf[i], acc[i][j], 0, 0, 0);
        }
        __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void *)out_img, 0, OH * OW * COUT, 0x00020000);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int gy = Y0 + 2 * w + i, gx = X0 + m;
            const bool ok = gy < OH && gx < OW;
#pragma unroll
            for (int j = 0; j < NG; j++) {
                const v16i a = acc[i][j];
                v4i v;
                v[0] = (int)pack4_relu7(a[0], a[1], a[2], a[3], act_floor & ACT_FLOOR_MASK);
                v[1] = (int)pack4_relu7(a[4], a[5], a[6], a[7], act_floor & ACT_FLOOR_MASK);
                v[2] = (int)pack4_relu7(a[8], a[9], a[10], a[11], act_floor & ACT_FLOOR_MASK);
                v[3] = (int)pack4_relu7(a[12], a[13], a[14], a[15], act_floor & ACT_FLOOR_MASK);
                const uint32_t off = ok ? tensor_offset(om, gy, gx, (uint32_t)j) + 16u * kh : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(v, ro, off, 0, 0);
            }
        }
        block_barrier();  // next patch complete, this patch free (raw barrier: the stores stay in flight)
    }
}

static_assert(L0_RAW_BYTES >= (L0_RAW_ROWS * L0_RAW_DW + 63) / 64 * 256, "k_l0: whole request instructions fit the raw buffer");

// Test hook: sicn_options.strip_chunks = n forces the number of vertical chunks a strip is cut into (the
// default heuristic gives small images one step per workgroup, which never exercises the rolling window).

size_t l0_bytes(int cout) { return (size_t)5 * cout * KSTEP; }

void pack_l0(const int8_t *w_okc, int cout, int8_t *dst)
{
    // w_okc: [cout][75], k = (ky*5+kx)*3 + c
    for (int ky = 0; ky < 5; ky++)
        for (int row = 0; row < cout; row++) {
            const int j = row >> 5, rho = row & 31;
            const int ch = j * 32 + 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3);
            int8_t logical[32];
            for (int s = 0; s < 8; s++)
                for (int c = 0; c < 4; c++)
                    logical[s * 4 + c] = (s < 5 && c < 3) ? w_okc[(size_t)ch * 75 + (ky * 5 + s) * 3 + c] : 0;
            const int g = (row >> 3) & 1;
            int8_t *t = dst + ((size_t)ky * cout + row) * 32;
            for (int h = 0; h < 2; h++)
                for (int b = 0; b < 16; b++) t[((h ^ g) << 4) + b] = logical[h * 16 + b];
        }
}

template <int NG>
static hipError_t launch_l0_groups(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out, int n_images, hipStream_t stream,
                                   int out_layout, const L0Plan &p, bool relu)
{
    const dim3 grid((unsigned)p.tiles_x, (unsigned)p.y_chunks, (unsigned)n_images);
    const size_t lds = 5 * 128 * KSTEP + 2 * L0_PATCH + 128 + L0_RAW_BYTES;
    hipError_t e = hipFuncSetAttribute((const void *)k_l0<4, NG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    // the nt policy follows the bytes of the whole tensor, as the consumer fetches it, whatever the groups stored here
    hipLaunchKernelGGL((k_l0<4, NG>), grid, dim3(256), lds, stream, in, out, w.d_w_l0, w.d_bias, g.IW, g.IH, g.OW, g.OH, p.tiles_y, p.ty_per,
                       out_layout,
                       (relu ? ACT_FLOOR_RELU : ACT_FLOOR_RAW) | (nt_store_wanted((size_t)g.OH * g.OW * g.COUT * n_images) ? ACT_NT_STORE : 0u));
    return hipGetLastError();
}

hipError_t launch_l0(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out,
                     int n_images, hipStream_t stream, int out_layout, const sicn_options &o, const ChipGeom &chip, bool relu, int groups)
{
    // runs of at most L0_CHUNK tiles (the LDS holds a run's pixels), evened out; small images: shorter runs, enough workgroups
    // (about four per CU, sicn_plan.h); the test hook (strip_chunks) can only shorten them
    const L0Plan p = plan_l0(g.OW, g.OH, n_images, false, o.strip_chunks, chip);
    if ((size_t)g.IH * g.IW * 3 * (size_t)n_images + 4 >= (size_t)OOB) return hipErrorInvalidValue;
    if ((size_t)g.OH * g.OW * g.COUT >= (size_t)OOB) return hipErrorInvalidValue;   // buffer-descriptor stores
    if (g.COUT != 128) return hipErrorInvalidValue;
    // three groups: only where a group is a plane of its own (in NHWC the fourth group is a quarter of every line)
    if (groups == 3 && out_layout == LAYOUT_GROUP) return launch_l0_groups<3>(g, w, in, out, n_images, stream, out_layout, p, relu);
    if (groups != 4) return hipErrorInvalidValue;
    return launch_l0_groups<4>(g, w, in, out, n_images, stream, out_layout, p, relu);
}

// =============================================================================================
// Layer 7 as tap products.  Input row i contributes to the output rows 2i-2 .. 2i+2 only (ky = 2i + 2 - oy), so a
// workgroup multiplies every input row ONCE and adds the products up across the rows afterwards (everything mod 256,
// bias and activation last).  Along x the layer stays a gather: for input row i and position x
//     T(i, x)[ky][px][c] = sum over dx, ch of in[i][x - 1 + dx][ch] * W[c][ky][2 dx - px][ch]
// is one column of a 30-row x 384-K matrix product (v_mfma_i32_16x16x64_i8: A = W'', 2 M tiles x 6 K steps, B = 16
// positions at three column shifts dx), and
//     out[2y    ][2x + px][c] = act(bias[c] + T(y - 1, x)[0] + T(y, x)[2] + T(y + 1, x)[4])
//     out[2y + 1][2x + px][c] = act(bias[c] +                  T(y, x)[1] + T(y + 1, x)[3]).
// A 16-position fragment is read from LDS 3 times per step (6 ds_read_b128, 12 MFMAs), not 9 times (18 and 18), and
// no MFMA row is spent on a (tap, phase) pair that is zero.
//   * W'' (12 KB) is held in REGISTERS (48 VGPRs) for the whole vertical strip a workgroup walks.  Row 4g + r of M
//     tile 0 / 1 (lane group g = lane >> 4 = 2 py + px holds rows 4g .. 4g+3 of a D tile):
//         tile 0, r < 3: (ky = 2 - py, px, c = r)          the lane's OWN output phase of row y = i
//         tile 1, r < 3: (ky = py ? 3 : 0, px, c = r)      py = 0: for row i + 1 (phase 0), py = 1: for row i - 1 (phase 1)
//         r = 3        : ky = 4 for row i - 1 (phase 0): c = 0 (tile 0) and 1 (tile 1) in the py = 0 groups, c = 2 (tile 0) in py = 1
//   * The strip is walked in steps of 4 input rows through the ROLLING LDS window: position P = r*36 + tx (r = row
//     counted from the top of the strip, 34 of the 36 columns used) sits at ring slot P mod 368.  While a step
//     computes, the 4 rows of the next step (exactly 9 pieces of 16 positions per region) are fetched by LDS-DMA:
//     every input row is fetched once per strip and the load latency is hidden behind a whole step.
//   * In step s wave w multiplies input row 4s + 1 + w (the four rows that landed last), writes the 18 product bytes
//     per position that belong to the rows above and below to a 3.5 KB LDS exchange area (packed, 3 bytes a dword),
//     and after ONE extra barrier adds what its neighbours wrote for its own row.  Waves 0 - 2 then hold the output
//     rows of y = 4s + 1 + w; wave 3's row 4s + 4 lacks the row below it until the next step, so wave 3 keeps its
//     partial sums in registers and finishes row 4s (from the step before) instead: a step stores the rows 4s .. 4s+3
//     as before.  Wave 3's bytes for the row below it cross the step in a slot that alternates with the step's parity.
//     A chunk starts with one step that stores nothing: it multiplies the rows 4 s_begin - 1 and 4 s_begin.
//   * Two LDS regions (K-group parity kg&1), each [slot][4 chunks x 16 B] with chunk
//     c2 = 2*half + (kg>>1) stored at c2 ^ ((P>>2)&3): a 16-lane ds_read_b128 group covers 16
//     distinct positions at ONE c2, i.e. 16 distinct 16-byte slots of a 256-byte LDS row.  Ring
//     wrap and step advance are multiples of 16 positions, so the XOR term is a lane constant.
//     Which channels a K byte stands for is free (W'' is packed to match): region R holds the
//     32-channel groups 2R, 2R+1 whole, so every LDS-DMA lane pair fetches one contiguous 32-byte
//     group entry (region-interleaved halves made each instruction use half of every line it touched).
//   * RGB output is transposed through a 384-byte per-wave LDS staging tile and stored as dwords
//     through a buffer descriptor (masked lanes = out of range), so a step always issues exactly
//     two stores and the wait for the prefetched rows is a counted vmcnt that leaves them in flight.
//   * k_l7<KH>: KH = 2 is all of the above.  k_l7<1> keeps region 0 only (L7Form below): half the requests, fragment reads and
//     MFMAs, for an input whose channels 64 .. 127 nobody wrote and no weight reads (launch_l7, halves = 1).
// =============================================================================================
constexpr int L7_AUX = 0;                                // cache policy of the input stream (2 = nt)
constexpr int L7_PITCH = 36;                             // positions per window row (34 used)
constexpr int L7_STEP_PIECES = L7_ROWS * L7_PITCH / 16;  // L7_ROWS = 4 input rows per step (sicn_plan.h): 9 LDS-DMA pieces per region per step
constexpr int L7_AHEAD = 1;                              // steps of rows in flight ahead of the step being computed
constexpr int L7_RING_PIECES = ((4 * L7_AHEAD + 6) * L7_PITCH + 15) / 16;   // 1 ahead: 23 pieces = 368 positions >= 10 rows
constexpr int L7_WGS = 3;                                // workgroups per CU the LDS ring allows (1 step ahead)
constexpr int L7_RING_POS = L7_RING_PIECES * 16;
constexpr int L7_REGION = L7_RING_PIECES * 1024;
constexpr int L7_STAGE = 2 * 192;                        // 2 output rows x 64 pixels x 3 B per wave
constexpr int L7_X1 = 2 * 256;                           // exchange, per wave: [position tile 2][lane 64] dwords = the rows r < 3 of M tile 1
constexpr int L7_X2 = 2 * 128;                           // exchange, per wave: [position tile 2][px 2][16 positions] dwords = the ky = 4 bytes
constexpr int L7_XCH = 5 * L7_X1 + 4 * L7_X2;            // wave 3's L7_X1 record twice (step parity)
constexpr int L7_MTILES = 2;
// Everything that follows from the number KH of live regions (64-channel halves of the input that are read at all).  KH = 2 is the
// kernel as described above.  KH = 1: the producing layer left its channels in the first half only (a wide layer of at most 4
// accumulator columns, sicn_live.h: column_of(pos) < 4 <=> pos < 64) and stored nothing into the planes of the groups 2, 3, whose
// weights are all zero: the ring is region 0 alone, a step requests 9 pieces, reads 3 fragments per position tile and runs 6 MFMAs.
template <int KH>
struct L7Form {
    static_assert(KH == 1 || KH == 2, "one or two 64-channel halves");
    static constexpr int LDS = KH * L7_REGION + 4 * L7_STAGE + 1024 + L7_XCH;
    static constexpr int KSTEPS = 3 * KH;                                   // W'': [M tile][K step = KH dx + half][row 16][64 B]
    static constexpr int PRO_N = (KH * 2 * L7_STEP_PIECES + 3) / 4;         // LDS-DMA instructions per wave: prologue (9 | 5)
    static constexpr int STEP_N = (KH * L7_STEP_PIECES + 3) / 4;            // and per step (5 | 3); the counted waits follow from it
    // the launch bound.  For KH = 1 it decides nothing: the kernel takes 92 VGPRs and 29 696 B of LDS, so five workgroups fit a CU
    // whatever is written here, and 3, 4 and 5 compile to the same instructions (profiles/l7_live_half_resource_usage.txt);
    // how many are resident is plan_l7's cut, just under two per CU
    static constexpr int WGS = L7_WGS;
};
static_assert(L7_ROWS * L7_PITCH % 16 == 0 && L7_RING_POS >= (4 * L7_AHEAD + 6) * L7_PITCH, "ring geometry");
static_assert(L7Form<2>::WGS * L7Form<2>::LDS <= 160 * 1024 && L7Form<1>::WGS * L7Form<1>::LDS <= 160 * 1024 && L7_XCH <= 4096,
              "workgroups per CU");
static_assert(L7Form<2>::LDS == 53248 && L7Form<2>::PRO_N == 9 && L7Form<2>::STEP_N == 5, "KH = 2 is the kernel it was");

// LDS-DMA pieces `first + 4i` (i < n) of a run of window rows: piece j < npieces covers region
// j / per_region, positions (j % per_region)*16 .. +15 of the run; row 0 of the run is input row iy0
// and lands at ring piece slot pslot0.  Only rows iy_min <= iy < iy_max (inside the image) are
// fetched, the rest is zero fill.  Every wave issues exactly N loads (the vmcnt bookkeeping of the
// caller depends on it): a piece index past the run becomes an out-of-range load into `scratch`.
// KH = 1: only region 0 exists, and stored chunk s of position P holds chunk c2 = 2*((s&1) ^ ((P>>2)&1)) + (s>>1), the inverse of
// what the readers of l7_body compute; lanes s and s^2 of a position fetch the two halves of one contiguous 32-byte group entry.
template <int N, int KH>
__device__ __forceinline__ void l7_load_rows(uint8_t *patch, uint8_t *scratch, const uint8_t *in_img, int in_img_bytes, int w,
                                             int lane, int per_region, int iy0, int iy_min, int iy_max, int pslot0, int X0,
                                             int IW, const TensorMap &tm)
{
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)in_img, 0, in_img_bytes, 0x00020000);
    // KH = 2: stored chunk (lane&3) of position P holds c2 ^ ((P>>2)&3); a piece starts at a multiple of 16 positions, so
    // (P>>2)&3 = (lane>>4)&3
    const int c2 = KH == 2 ? (lane & 3) ^ ((lane >> 4) & 3) : 2 * ((lane & 1) ^ ((lane >> 4) & 1)) + ((lane >> 1) & 1);
#pragma unroll
    for (int i = 0; i < N; i++) {
        const int j = w + 4 * i;
        const bool real = j < KH * per_region;   // wave-uniform
        const int region = (KH == 2 && j >= per_region) ? 1 : 0, kk = j - region * per_region;
        const int q = kk * 16 + (lane >> 2);
        const int row = q / L7_PITCH, tx = q - row * L7_PITCH;
        const int iy = iy0 + row, ix = X0 - 1 + tx;
        const bool ok = real && tx < TILE_X + 2 && iy >= iy_min && iy < iy_max && ix >= 0 && ix < IW;
        // region R keeps channel groups 2R, 2R+1 whole: chunk c2 = 16 bytes (c2&1) of group 2R + (c2>>1), so
        // a lane pair fetches one contiguous 32-byte group entry and a piece reads whole 512-byte runs
        const uint32_t off = ok ? tensor_offset(tm, iy, ix, (uint32_t)(2 * region + (c2 >> 1))) + 16u * (c2 & 1) : OOB;
        int slot = pslot0 + kk;
        slot = slot >= L7_RING_PIECES ? slot - L7_RING_PIECES : slot;
        uint8_t *dst = real ? patch + region * L7_REGION + slot * 1024 : scratch;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, LDS_PTR(dst), 16, off, 0, 0, L7_AUX);
    }
}

template <int KH>
__device__ __forceinline__ void l7_body(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const int8_t *__restrict__ w_l7,
                                        const int8_t *__restrict__ bias, int IW, int IH, int OW, int OH, int steps_y, int y_chunks,
                                        int tiles_x, int n_images, int in_layout, int n_xcd)
{
    constexpr int CIN = 128;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *patch = smem;
    using F = L7Form<KH>;
    uint8_t *stage = smem + KH * L7_REGION;
    uint8_t *scratch = stage + 4 * L7_STAGE;   // 1 KiB sink of the padding loads
    uint8_t *xch1 = scratch + 1024;            // 5 records of L7_X1
    uint8_t *xch2 = xch1 + 5 * L7_X1;          // 4 records of L7_X2

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    // logical work list: strip (fastest), chunk, image — an XCD gets whole rows of neighbouring strips
    const int item = xcd_logical_index(tiles_x * y_chunks * n_images, n_xcd);
    if (item < 0) return;
    const int bx = item % tiles_x, by = (item / tiles_x) % y_chunks, img = item / (tiles_x * y_chunks);
    const int X0 = bx * TILE_X;
    const int per = (steps_y + y_chunks - 1) / y_chunks;
    const int s_begin = by * per, s_end = min(steps_y, s_begin + per);
    if (s_begin >= s_end) return;  // before any LDS-DMA is issued

    // lane roles in v_mfma_i32_16x16x64_i8: A row / B column = lane & 15, K bytes 16*(lane>>4)..+15
    const int m = lane & 15, kg = lane >> 4;
    v4i wf[L7_MTILES * F::KSTEPS];
#pragma unroll
    for (int s = 0; s < L7_MTILES * F::KSTEPS; s++) wf[s] = *(const v4i *)(w_l7 + (s * 16 + m) * 64 + kg * 16);
    const int b0 = bias[0], b1 = bias[1], b2 = bias[2];

    const int in_img_bytes = IH * IW * CIN;
    const uint8_t *in_img = in + (size_t)img * in_img_bytes;
    uint8_t *out_img = out + (size_t)img * OH * OW * 3;
    const int py = kg >> 1, px = kg & 1;
    uint8_t *my_stage = stage + w * L7_STAGE;
    const bool fast_rows = ((OW * 3) & 3) == 0 && X0 + TILE_X <= IW;

    // window row r <-> input row 4*s_begin - 3 + r; rows 0,1 are never fetched (they only make the
    // prologue a whole number of pieces and read as zeros)
    const int iy_top = 4 * s_begin - 3;
    const int iy_max = min(IH, 4 * s_end + 1);   // last row this chunk reads
    const TensorMap tm = tensor_map(in_layout, CIN, IW, IH);
    l7_load_rows<F::PRO_N, KH>(patch, scratch, in_img, in_img_bytes, w, lane, 2 * L7_STEP_PIECES, iy_top, max(iy_top + 2, 0), iy_max, 0, X0,
                    IW, tm);
    // block k = window rows 4k+4 .. 4k+7 = the rows step k adds; blocks 1 .. AHEAD-1 start now
    int pnext = 2 * L7_STEP_PIECES;        // ring piece slot of the next block to be requested
    int ynext = iy_top + 8;                // its first input row
#pragma unroll
    for (int k = 1; k < L7_AHEAD; k++) {
        l7_load_rows<F::STEP_N, KH>(patch, scratch, in_img, in_img_bytes, w, lane, L7_STEP_PIECES, ynext, 0, iy_max, pnext, X0, IW, tm);
        ynext += L7_ROWS;
        pnext += L7_STEP_PIECES;
        pnext = pnext >= L7_RING_PIECES ? pnext - L7_RING_PIECES : pnext;
    }

    // per-lane fragment addressing: step t multiplies window row 4t + 4 + w, P = (4t + 4 + w)*36 + 16c + m + dx
    auto frag_a = [&](int dx) { return (uint32_t)((4 + w) * L7_PITCH + m + dx); };
    // KH = 1: one K step of 64 bytes is the region's 64 channels, lane group kg reads chunk c2 = kg (channels 16 kg .. 16 kg + 15:
    // K byte b is channel b).  ds_read_b128 is served in lane groups that pair the m-complementary halves of kg = 2h and 2h + 1
    // (lanes 0-3, 12-15 with 20-27, ...): 16 distinct positions, but two chunks.  So the chunk is stored at
    // 2*(c2&1) + ((c2>>1) ^ ((P>>2)&1)) (not at c2 ^ ((P>>2)&3), which puts the two kg of a pair on the same banks): of the four
    // positions of a lane group that share P&3 (one 64-byte quarter of a 256-byte LDS row), (P>>2)&3 runs through x, x+1, x+2, x+3
    // with kg parity e, o, o, e or o, e, e, o; the two lanes of equal parity differ in (P>>2)&1 and the parities take different slot
    // pairs, so the 16 lanes hit 16 distinct 16-byte slots whatever the alignment of the fragment.  Like the KH = 2 term it is a lane
    // constant (ring wrap and step advance are multiples of 16 positions).
    auto frag_s = [&](uint32_t a) {
        return KH == 2 ? (uint32_t)((kg & 1) * L7_REGION) + ((((uint32_t)(kg >> 1)) ^ ((a >> 2) & 3u)) << 4)
                       : (2u * (uint32_t)(kg & 1) + (((uint32_t)(kg >> 1)) ^ ((a >> 2) & 1u))) << 4;
    };
    uint32_t fa[3], fs[3];
#pragma unroll
    for (int dx = 0; dx < 3; dx++) {
        fa[dx] = frag_a(dx);
        fs[dx] = frag_s(fa[dx]);
    }
    // exchange: who multiplied the rows above and below this wave's output row
    const int w_below = (w + 1) & 3;
    const uint32_t x1_lane = (uint32_t)lane * 4u, x2_lane = (uint32_t)(px * 16 + m) * 4u;
    int saved[2][3] = {{0, 0, 0}, {0, 0, 0}};   // wave 3: row 4s + 4 without the row below it
    wait_vmcnt<F::STEP_N * (L7_AHEAD - 1)>();
    block_barrier();

    // the first pass (s = s_begin - 1) stores nothing and requests nothing: its rows 4 s_begin - 1 and 4 s_begin came with the prologue
    int base = L7_RING_POS - L7_ROWS * L7_PITCH;   // (144 t) mod ring: ring slot of window row 4t, column 0
    for (int s = s_begin - 1; s < s_end; s++) {
        const bool live = s >= s_begin;    // wave-uniform
        const int par = (s - s_begin) & 1;
        const int Y = 4 * s;               // first output row pair of this step
        // always issued in a live step (rows past the chunk are zero fill): the counted waits below rely on it
        if (live) {
            l7_load_rows<F::STEP_N, KH>(patch, scratch, in_img, in_img_bytes, w, lane, L7_STEP_PIECES, ynext, 0, iy_max, pnext, X0, IW, tm);
            ynext += L7_ROWS;
        }

        v4i acc[2][L7_MTILES];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            acc[c][0] = v4i{b0, b1, b2, 0};    // C row 4*kg + r of M tile 0 = this lane's own phase, channel r
            acc[c][1] = v4i{0, 0, 0, 0};
#pragma unroll
            for (int dx = 0; dx < 3; dx++) {
                uint32_t slot = (uint32_t)base + fa[dx] + 16u * c;
                slot = min(slot, slot - (uint32_t)L7_RING_POS);   // one wrap at most
                const uint32_t addr = slot * 64u + fs[dx];
                const v4i p0 = *(const v4i *)(patch + addr);
                if constexpr (KH == 2) {
                    const v4i p1 = *(const v4i *)(patch + (addr ^ 32u));   // the other 32-channel group of each region: c2 ^ 2
#pragma unroll
                    for (int t = 0; t < L7_MTILES; t++) {
                        acc[c][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[t * F::KSTEPS + dx * 2 + 0], p0, acc[c][t], 0, 0, 0);
                        acc[c][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[t * F::KSTEPS + dx * 2 + 1], p1, acc[c][t], 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < L7_MTILES; t++)
                        acc[c][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[t * F::KSTEPS + dx], p0, acc[c][t], 0, 0, 0);
                }
            }
        }
        // ---- products for the neighbouring rows -> exchange --------------------------------------
        {
            uint8_t *x1 = xch1 + (w == 3 ? 3 + par : w) * L7_X1, *x2 = xch2 + w * L7_X2;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const uint32_t lo = __builtin_amdgcn_perm((uint32_t)acc[c][1][1], (uint32_t)acc[c][1][0], 0x0c0c0400u);
                *(uint32_t *)(x1 + c * 256 + x1_lane) = __builtin_amdgcn_perm((uint32_t)acc[c][1][2], lo, 0x0c040100u);
                // ky = 4: bytes 0, 1 from the py = 0 lane (c = 0, 1), bytes 2, 3 from the py = 1 lane (c = 2, zero)
                *(uint16_t *)(x2 + c * 128 + x2_lane + 2 * py) =
                    (uint16_t)__builtin_amdgcn_perm((uint32_t)acc[c][1][3], (uint32_t)acc[c][0][3], 0x0c0c0400u);
            }
        }
        block_barrier();   // the four rows' products are in the exchange
        // ---- sums across the rows (low bytes count, the rest is dropped by the pack) --------------
        int fin[2][3];
        {
            // py = 0: ky = 0 of the row above and ky = 4 of the row below; py = 1: ky = 3 of the row below
            const int w_above1 = w == 0 ? 3 + (par ^ 1) : w - 1, w_below1 = w_below == 3 ? 3 + par : w_below;
            const uint8_t *x1 = xch1 + (py ? w_below1 : w_above1) * L7_X1, *x2 = xch2 + w_below * L7_X2;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const uint32_t r1 = *(const uint32_t *)(x1 + c * 256 + x1_lane);
                const uint32_t r2 = *(const uint32_t *)(x2 + c * 128 + x2_lane);
                const uint32_t above = py ? 0u : r1, below = py ? r1 : r2;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int cur = acc[c][0][k] + (int)(above >> (8 * k));
                    const int mine = w == 3 ? saved[c][k] : cur;
                    saved[c][k] = cur;
                    fin[c][k] = mine + (int)(below >> (8 * k));
                }
            }
        }
        // ---- epilogue ----------------------------------------------------------------------
        const int gy = Y + w_below;        // wave 3 finishes the row it kept from the step before
        if (fast_rows) {
            // stage [2 rows = py][64 pixels = 2*(16c+m)+px][3] and write the rows as dwords
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const uint32_t v = pack4_relu7(fin[c][0], fin[c][1], fin[c][2], 0);
                uint8_t *d = my_stage + py * 192 + (2 * (16 * c + m) + px) * 3;
                d[0] = (uint8_t)v;
                d[1] = (uint8_t)(v >> 8);
                d[2] = (uint8_t)(v >> 16);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private staging: no barrier needed
            __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void *)out_img, 0, OH * OW * 3, 0x00020000);
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int idx = k * 64 + lane;                   // dword index in the 2 x 48 tile
                const int row = idx >= 48 ? 1 : 0, col = idx - 48 * row;
                const bool ok = live && idx < 96 && gy < IH;
                const uint32_t v = *(const uint32_t *)(my_stage + (idx < 96 ? idx : 0) * 4);
                const uint32_t off = ok ? (uint32_t)(((2 * gy + row) * OW + 2 * X0) * 3 + col * 4) : OOB;
                __builtin_amdgcn_raw_buffer_store_b32(v, ro, off, 0, 0);
            }
            // leave in flight: this step's 2 stores and the AHEAD-1 younger row blocks (STEP_N loads + 2 stores each)
            wait_vmcnt<2 + (F::STEP_N + 2) * (L7_AHEAD - 1)>();
        } else {
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const int gx = X0 + 16 * c + m;
                if (live && gy < IH && gx < IW) {
                    const uint32_t v = pack4_relu7(fin[c][0], fin[c][1], fin[c][2], 0);
                    uint8_t *dst = out_img + ((size_t)(2 * gy + py) * OW + 2 * gx + px) * 3;
                    dst[0] = (uint8_t)v;
                    dst[1] = (uint8_t)(v >> 8);
                    dst[2] = (uint8_t)(v >> 16);
                }
            }
            wait_vmcnt<0>();
        }
        block_barrier();   // next rows landed for every wave, this step's rows and the exchange are free
        base += L7_ROWS * L7_PITCH;
        base = base >= L7_RING_POS ? base - L7_RING_POS : base;
        if (live) {
            pnext += L7_STEP_PIECES;
            pnext = pnext >= L7_RING_PIECES ? pnext - L7_RING_PIECES : pnext;
        }
    }
    wait_vmcnt<0>();   // the zero-fill tail of the prefetch must land before the LDS is released
}
template <int KH>
__global__ __launch_bounds__(256, L7Form<KH>::WGS) void k_l7(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const int8_t *__restrict__ w_l7,
                                                    const int8_t *__restrict__ bias, int IW, int IH, int OW, int OH, int steps_y, int y_chunks,
                                                    int tiles_x, int n_images, int in_layout, int n_xcd)
{
    l7_body<KH>(in, out, w_l7, bias, IW, IH, OW, OH, steps_y, y_chunks, tiles_x, n_images, in_layout, n_xcd);
}

size_t l7_bytes(int cin) { return (size_t)L7_MTILES * L7Form<2>::KSTEPS * 16 * 64 * (cin / 128); }
size_t l7_half_bytes() { return (size_t)L7_MTILES * L7Form<1>::KSTEPS * 16 * 64; }

void pack_l7(const int8_t *w_okc, int cin, int8_t *dst)
{
    // w_okc: [3][25*cin]; dst: [M tile 2][K step 2 dx + half][row 16][64 B]; row = 4*(2 py + px) + r (see the head of this section)
    for (int tile = 0; tile < L7_MTILES; tile++)
        for (int dx = 0; dx < 3; dx++)
            for (int half = 0; half < 2; half++)
                for (int row = 0; row < 16; row++) {
                    const int g = row >> 2, r = row & 3, py = g >> 1, px = g & 1;
                    int ky, c;
                    if (r < 3) {
                        ky = tile == 0 ? 2 - py : (py ? 3 : 0);
                        c = r;
                    } else {
                        ky = 4;
                        c = py ? (tile == 0 ? 2 : -1) : tile;
                    }
                    const int kx = 2 * dx - px;
                    int8_t *t = dst + ((((size_t)tile * 3 + dx) * 2 + half) * 16 + row) * 64;
                    // K byte b of step `half` is read by lane group kg = b>>4 from LDS region kg&1, chunk
                    // 2*half + (kg>>1): channel 64*(kg&1) + 32*half + 16*(kg>>1) + (b&15)   (see l7_load_rows)
                    for (int b = 0; b < 64; b++) {
                        const int kg = b >> 4, ch = 64 * (kg & 1) + 32 * half + 16 * (kg >> 1) + (b & 15);
                        t[b] = (c >= 0 && kx >= 0 && kx < 5) ? w_okc[(size_t)c * 25 * cin + (ky * 5 + kx) * cin + ch] : 0;
                    }
                }
}

void pack_l7_half(const int8_t *w_okc, int8_t *dst)
{
    // w_okc: [3][25*128]; dst: [M tile 2][dx 3][row 16][64 B]; the rows are those of pack_l7 (row = 4*(2 py + px) + r), one K step per dx
    for (int tile = 0; tile < L7_MTILES; tile++)
        for (int dx = 0; dx < 3; dx++)
            for (int row = 0; row < 16; row++) {
                const int g = row >> 2, r = row & 3, py = g >> 1, px = g & 1;
                int ky, c;
                if (r < 3) {
                    ky = tile == 0 ? 2 - py : (py ? 3 : 0);
                    c = r;
                } else {
                    ky = 4;
                    c = py ? (tile == 0 ? 2 : -1) : tile;
                }
                const int kx = 2 * dx - px;
                int8_t *t = dst + (((size_t)tile * 3 + dx) * 16 + row) * 64;
                // K byte b is read by lane group kg = b>>4 from LDS region 0, chunk kg = bytes 16*(kg&1) .. of the 32-channel group
                // kg>>1: channel b (see l7_load_rows); the channels 64 .. 127 have no K byte, their weights are zero by the plan
                for (int b = 0; b < 64; b++)
                    t[b] = (c >= 0 && kx >= 0 && kx < 5) ? w_okc[(size_t)c * 25 * 128 + (ky * 5 + kx) * 128 + b] : 0;
            }
}

template <int KH>
static hipError_t launch_l7_form(const LayerGeom &g, const int8_t *w_img, const sicn_weights &w, const uint8_t *in, uint8_t *out, int n_images,
                                 hipStream_t stream, int in_layout, const L7Plan &p, const ChipGeom &chip)
{
    const size_t lds = L7Form<KH>::LDS;
    hipError_t e = hipFuncSetAttribute((const void *)k_l7<KH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_l7<KH>, dim3(p.grid_x), dim3(256), lds, stream, in, out, w_img, w.d_bias, g.IW, g.IH, g.OW, g.OH, p.steps_y, p.y_chunks,
                       p.tiles_x, n_images, in_layout, chip.n_xcd);
    return hipGetLastError();
}

// halves = 1: the channels 64 .. 127 of the input are neither read nor multiplied (the caller knows that their weights are zero and
// that the layout keeps every 32-channel group in a plane of its own)
hipError_t launch_l7(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out,
                     int n_images, hipStream_t stream, int in_layout, const sicn_options &o, const ChipGeom &chip, int halves)
{
    if (g.CIN != 128 || g.COUT != 3) return hipErrorInvalidValue;
    if (halves == 1 && (in_layout == LAYOUT_NHWC || !w.d_w_l7_half)) return hipErrorInvalidValue;
    if ((size_t)g.IH * g.IW * g.CIN >= (size_t)OOB) return hipErrorInvalidValue;
    if ((size_t)g.OH * g.OW * 3 >= (size_t)OOB) return hipErrorInvalidValue;   // buffer-descriptor stores
    // about two workgroups per CU in all (three would fit) — measured
    // r02 (tools/strip_sweep.py): 1080p x 1 best at 16 - 24 chunks of 30 strips, x 4 at 4 - 6 of 120, 4K x 8 at 1 of 480;
    // every extra chunk re-fetches six halo rows, re-loads the 12 KB of weights and multiplies the two rows above it once more
    // (r03, re-measured on one 1080p image, 30 strips: 13 / 15 / 17 / 19 / 21 / 25 chunks -> 23 / 22 / 19 / 24 / 23 / 21 us: the best
    // cut is the one that stays just under TWO workgroups per CU, 510 of 512; the 640 of round 2 was the middle of a flat region)
    const L7Plan p = plan_l7(g.IW, g.IH, n_images, o.strip_chunks, chip);
    return halves == 1 ? launch_l7_form<1>(g, w.d_w_l7_half, w, in, out, n_images, stream, in_layout, p, chip)
                       : launch_l7_form<2>(g, w.d_w_l7, w, in, out, n_images, stream, in_layout, p, chip);
}

}  // namespace sicn
