// The tile bodies of the packed-K RGB ends of a ragged net (k_ragged_rgb.hip): conv 3 -> N and deconv N -> 3 on
// v_mfma_i32_16x16x64_i8, each a function of ONE image like any_tile() (k_any_body.hpp), whose zero-padded RGB ends they replace.
// The K layouts and the weight images are described in ragged_rgb_host.hpp.
//
// Conv: one 16 x 16 tile of output positions, every block of 64 output channels in a loop over the ONE patch.  The 35 x 35 input
// pixels are read from the image's raw bytes and expanded to RGBX dwords in LDS: 36 rows of 40 pixel slots (row 35 and the slots
// 35 .. 39 are met by zero weights only).  Lane (col, g) of K step s reads the 16 bytes of pixels 2 col + 4 (g & 1) .. + 3 of patch
// row 2 ly + 2 s + (g >> 1) as two 8-byte reads at an 8-byte aligned address.
// An image of a ragged RGB tensor starts at any byte phase and so does each of its rows: the bytes are loaded as aligned dwords and
// re-aligned in registers (l0_expand of k_l0_common.hpp does the same from LDS).  A dword is loaded only where it overlaps the
// tensor [t0, t1): with a 4-byte aligned tensor NO LOAD TOUCHES A BYTE BEYOND THE TENSOR'S SIZE ROUNDED UP TO A MULTIPLE OF 4 — the
// allowance k_l0 takes — and none before its first byte.
//
// Deconv: one 16 x 16 tile of INPUT positions with all four phases.  The 18 x 18 x 64 patch of a K chunk is staged once, as
// any_tile stages it; nine tap offsets; lane (col, g) of the C/D layout then holds the three channels of phase g at position col
// and stores 3 bytes to output pixel (2 my + (g >> 1), 2 mx + (g & 1)).  Byte stores only: the neighbouring pixels belong to other
// lanes, tiles and images.
//
// Both have a PLANAR sibling (include/sicn_ragged_planar.h; k_rgb_conv_ragged_planar and k_rgb_deconv_ragged_planar of
// k_ragged_rgb.hip): the conv with another loader in front of the same rgb_conv_mma, the deconv with another epilogue
// (rgb_deconv_tile<true>).
#pragma once
#include "k_any_body.hpp"
#include "ragged_planar_host.hpp"
#include "ragged_rect_host.hpp"
#include "ragged_rgb_host.hpp"

namespace sicn {

constexpr int RGBC_PX = 40;                          // pixel slots per patch row: 2 * 15 + 4 + 4 = 38 are read
constexpr int RGBC_PITCH = RGBC_PX * 4;              // 160 bytes
constexpr int RGBC_ROWS = ANY_CONV_EDGE + 1;         // 36: K step 2 reads kernel row 5 (zero weights)
constexpr int RGBC_QUADS = RGBC_ROWS * (RGBC_PX / 4);
constexpr int RGBC_LDS = RGBC_ROWS * RGBC_PITCH;     // 5760 bytes
constexpr int RGBD_LDS = ANY_DECONV_EDGE * ANY_DECONV_EDGE * 64;   // 20736 bytes

// Everything behind the patch, which every wave sees in smem (RGBC_LDS bytes of RGBX dwords): the B fragments, the three K steps, the
// loop over the blocks J0, J0 + Jstep, ... of 64 output channels and the epilogue.  om: the image's own [OH][OW][O] output.
__device__ __forceinline__ void rgb_conv_mma(uint8_t *__restrict__ om, const int8_t *__restrict__ wimg, const int8_t *__restrict__ bias,
                                             int OW, int OH, int O, int y0, int x0, int J0, int Jstep, uint32_t floor2,
                                             const uint8_t *smem)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = lane & 15, g = lane >> 4;

    // ---- the B fragments of the wave's four rows, all three K steps: read once, used for every block of channels
    v4i bf[RGB_CONV_KSTEPS][4];
#pragma unroll
    for (int s = 0; s < RGB_CONV_KSTEPS; s++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint8_t *p = smem + (2 * (4 * wv + c) + 2 * s + (g >> 1)) * RGBC_PITCH + 8 * col + 16 * (g & 1);
            const uint2 a = *reinterpret_cast<const uint2 *>(p), b = *reinterpret_cast<const uint2 *>(p + 8);
            bf[s][c] = v4i{(int)a.x, (int)a.y, (int)b.x, (int)b.y};
        }

    const int nblk = (O + 63) >> 6;
#pragma unroll 1
    for (int J = J0; J < nblk; J += Jstep) {
        v4i acc[4][4];                                          // [row c][tile j], from the bias
#pragma unroll
        for (int j = 0; j < 4; j++) {
            v4i b;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 64 * J + 16 * g + 4 * j + r;
                b[r] = o < O ? (int)bias[o] : 0;
            }
#pragma unroll
            for (int c = 0; c < 4; c++) acc[c][j] = b;
        }
        const int8_t *wt = wimg + (size_t)J * RGB_CONV_KSTEPS * 4 * 1024 + col * 64 + 16 * g;
#pragma unroll
        for (int s = 0; s < RGB_CONV_KSTEPS; s++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const v4i af = *reinterpret_cast<const v4i *>(wt + (s * 4 + j) * 1024);
#pragma unroll
                for (int c = 0; c < 4; c++) acc[c][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[s][c], acc[c][j], 0, 0, 0);
            }
        // ---- any_tile's epilogue: 16 consecutive channels of one pixel per lane
        const int o0 = 64 * J + 16 * g;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int my = y0 + 4 * wv + c, mx = x0 + col;
            if (my >= OH || mx >= OW || o0 >= O) continue;    // N % 16 == 0: the lane's 16 channels are all real or all padding
            uint4 q;
            q.x = pack4_relu7(acc[c][0][0], acc[c][0][1], acc[c][0][2], acc[c][0][3], floor2);
            q.y = pack4_relu7(acc[c][1][0], acc[c][1][1], acc[c][1][2], acc[c][1][3], floor2);
            q.z = pack4_relu7(acc[c][2][0], acc[c][2][1], acc[c][2][2], acc[c][2][3], floor2);
            q.w = pack4_relu7(acc[c][3][0], acc[c][3][1], acc[c][3][2], acc[c][3][3], floor2);
            *reinterpret_cast<uint4 *>(om + ((size_t)my * OW + mx) * O + o0) = q;
        }
    }
}

// im / om: the image's own [IH][IW][3] input and [OH][OW][O] output; [t0, t1): the whole input tensor; (y0, x0): the tile's origin in
// output positions; blocks J0, J0 + Jstep, ... of 64 output channels; smem: RGBC_LDS bytes, 16-byte aligned
__device__ __forceinline__ void rgb_conv_tile(const uint8_t *__restrict__ im, const uint8_t *t0, const uint8_t *t1, uint8_t *__restrict__ om,
                                              const int8_t *__restrict__ wimg, const int8_t *__restrict__ bias, int IW, int IH, int OW,
                                              int OH, int O, int y0, int x0, int J0, int Jstep, uint32_t floor2, uint8_t *smem)
{
    const int tid = threadIdx.x;

    // ---- the patch: a quad = 4 pixels of one patch row = 12 bytes from byte phase sh of four aligned dwords
    const uintptr_t lo = (uintptr_t)t0, hi = (uintptr_t)t1;
#pragma unroll
    for (int q0 = 0; q0 < RGBC_QUADS; q0 += 256) {
        const int q = q0 + tid;
        if (q >= RGBC_QUADS) break;
        const int r = q / (RGBC_PX / 4), gq = q - r * (RGBC_PX / 4);
        const int iy = 2 * y0 - 2 + r, ix = 2 * x0 - 2 + 4 * gq;
        uint4 v = uint4{0u, 0u, 0u, 0u};
        if (iy >= 0 && iy < IH && ix + 3 >= 0 && ix < IW) {
            const uint8_t *p = im + ((int64_t)iy * IW + ix) * 3;                        // ix < 0: up to 6 bytes before the row
            const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
            const uint8_t *p0 = p - sh;
            uint32_t d[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uintptr_t A = (uintptr_t)(p0 + 4 * k);
                d[k] = (A + 4 > lo && A < hi) ? *reinterpret_cast<const uint32_t *>(p0 + 4 * k) : 0u;
            }
            const uint32_t w0 = __builtin_amdgcn_alignbyte(d[1], d[0], sh);
            const uint32_t w1 = __builtin_amdgcn_alignbyte(d[2], d[1], sh);
            const uint32_t w2 = __builtin_amdgcn_alignbyte(d[3], d[2], sh);
            v.x = (ix + 0 >= 0 && ix + 0 < IW) ? (w0 & 0xFFFFFFu) : 0u;
            v.y = (ix + 1 >= 0 && ix + 1 < IW) ? (__builtin_amdgcn_alignbyte(w1, w0, 3) & 0xFFFFFFu) : 0u;
            v.z = (ix + 2 >= 0 && ix + 2 < IW) ? (__builtin_amdgcn_alignbyte(w2, w1, 2) & 0xFFFFFFu) : 0u;
            v.w = (ix + 3 >= 0 && ix + 3 < IW) ? (w2 >> 8) : 0u;
        }
        *reinterpret_cast<uint4 *>(smem + q * 16) = v;
    }
    __syncthreads();
    rgb_conv_mma(om, wimg, bias, OW, OH, O, y0, x0, J0, Jstep, floor2, smem);
}

// rgb_conv_tile over a PLANAR image: im = its three planes [3][IH][IW].  Only the loader differs (planar_quad, ragged_planar_host.hpp).
__device__ __forceinline__ void rgb_conv_tile_planar(const uint8_t *__restrict__ im, const uint8_t *t0, const uint8_t *t1,
                                                     uint8_t *__restrict__ om, const int8_t *__restrict__ wimg,
                                                     const int8_t *__restrict__ bias, int IW, int IH, int OW, int OH, int O, int y0, int x0,
                                                     int J0, int Jstep, uint32_t floor2, uint8_t *smem)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int q0 = 0; q0 < RGBC_QUADS; q0 += 256) {
        const int q = q0 + tid;
        if (q >= RGBC_QUADS) break;
        const int r = q / (RGBC_PX / 4), gq = q - r * (RGBC_PX / 4);
        const PlanarQuad v = planar_quad((uintptr_t)im, IW, IH, 2 * y0 - 2 + r, 2 * x0 - 2 + 4 * gq, (uintptr_t)t0, (uintptr_t)t1,
                                         [](uintptr_t a) { return *reinterpret_cast<const uint32_t *>(a); });
        *reinterpret_cast<uint4 *>(smem + q * 16) = uint4{v.px[0], v.px[1], v.px[2], v.px[3]};
    }
    __syncthreads();
    rgb_conv_mma(om, wimg, bias, OW, OH, O, y0, x0, J0, Jstep, floor2, smem);
}

// im / om: the image's own [IH][IW][C] input and [2 IH][OW = 2 IW][3] output; (y0, x0): the tile's origin in input positions;
// smem: RGBD_LDS bytes, 16-byte aligned.  OH is not read.
// PLANAR: om = the image's planes [3][OH][OW] cut to 1 <= OW <= 2 IW, 1 <= OH <= 2 IH (include/sicn_ragged_planar.h).  Only the
// epilogue differs: the lane stores one byte into each plane where its pixel lies inside the cut; the pixels outside are computed
// and not stored.  Across the 16 lanes of a row group the bytes of a plane are 2 apart and the phase g & 1 fills the gaps: 32
// consecutive bytes per plane.
// RECT (include/sicn_ragged_rect.h): om = the image's own 3 OH OW bytes, [OH][OW][3] or planes [3][OH][OW], which hold the rectangle
// (RX0, RY0, OW, OH) of the [2 IH][2 IW] reconstruction.  Again only the epilogue differs (ragged_rect_host.hpp): a pixel is stored iff
// it is inside the rectangle, at the address its in-rectangle coordinates give.  The caller has returned already where the tile's
// 32 x 32 output pixels do not meet the rectangle.
template <bool PLANAR, bool RECT = false>
__device__ __forceinline__ void rgb_deconv_tile(const uint8_t *__restrict__ im, uint8_t *__restrict__ om, const int8_t *__restrict__ wimg,
                                                const int8_t *__restrict__ bias, int IW, int IH, int C, int OW, int OH, int y0, int x0,
                                                uint32_t floor2, uint8_t *smem, int32_t RX0 = 0, int32_t RY0 = 0)
{
    constexpr int EDGE = ANY_DECONV_EDGE;
    constexpr int UNITS = EDGE * EDGE * 4;                     // 16-byte units of one chunk's patch
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int nchunk = (C + 63) >> 6;
    const int iy0 = y0 - 1, ix0 = x0 - 1;                      // input pixel of patch pixel (0, 0)

    v4i acc[4];                                                 // rows 4 g + c: bias[c] of phase g, row 4 g + 3 stays 0
    {
        const v4i b = v4i{(int)bias[0], (int)bias[1], (int)bias[2], 0};
#pragma unroll
        for (int c = 0; c < 4; c++) acc[c] = b;
    }

    for (int n = 0; n < nchunk; n++) {
        if (n) __syncthreads();                                 // every wave is done with the previous chunk's patch
#pragma unroll 1
        for (int u0 = 0; u0 < UNITS; u0 += 3 * 256) {
            uint4 v[3];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const int u = u0 + i * 256 + tid;
                v[i] = uint4{0u, 0u, 0u, 0u};
                if (u < UNITS) {
                    const int pp = u >> 2, c0 = n * 64 + 16 * (u & 3);
                    const int pr = pp / EDGE, pc = pp - pr * EDGE;
                    const int iy = iy0 + pr, ix = ix0 + pc;
                    if (iy >= 0 && iy < IH && ix >= 0 && ix < IW && c0 < C)     // C % 32 == 0: the unit is all inside the pixel
                        v[i] = *reinterpret_cast<const uint4 *>(im + ((size_t)iy * IW + ix) * C + c0);
                }
            }
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const int u = u0 + i * 256 + tid;
                if (u < UNITS) *reinterpret_cast<uint4 *>(smem + (size_t)u * 16) = v[i];
            }
        }
        __syncthreads();

        // ---- nine offsets: the six patch rows the wave's four rows meet, one column offset at a time
#pragma unroll
        for (int dx = 0; dx < 3; dx++) {
            v4i bf[6];
#pragma unroll
            for (int k = 0; k < 6; k++)
                bf[k] = *reinterpret_cast<const v4i *>(smem + (size_t)((4 * wv + k) * EDGE + col + dx) * 64 + 16 * g);
#pragma unroll
            for (int dy = 0; dy < 3; dy++) {
                const v4i af = *reinterpret_cast<const v4i *>(wimg + (((size_t)(dy * 3 + dx) * nchunk + n) * 16 + col) * 64 + 16 * g);
#pragma unroll
                for (int c = 0; c < 4; c++) acc[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[c + dy], acc[c], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: the lane's own three bytes of output pixel (2 my + (g >> 1), 2 mx + (g & 1))
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int my = y0 + 4 * wv + c, mx = x0 + col;
        if constexpr (RECT) {
            const int oy = 2 * my + (g >> 1), ox = 2 * mx + (g & 1);
            if (!rect_stored(oy, ox, 2 * IW, 2 * IH, RX0, RY0, OW, OH)) continue;
            const uint32_t ry = rect_rel(oy, RY0), rx = rect_rel(ox, RX0);
            const uint32_t q = pack4_relu7(acc[c][0], acc[c][1], acc[c][2], acc[c][3], floor2);
            om[rect_at<PLANAR>(0, ry, rx, OW, OH)] = (uint8_t)q;
            om[rect_at<PLANAR>(1, ry, rx, OW, OH)] = (uint8_t)(q >> 8);
            om[rect_at<PLANAR>(2, ry, rx, OW, OH)] = (uint8_t)(q >> 16);
        } else if constexpr (PLANAR) {
            const int oy = 2 * my + (g >> 1), ox = 2 * mx + (g & 1);
            if (!planar_stored(oy, ox, OW, OH)) continue;
            const uint32_t q = pack4_relu7(acc[c][0], acc[c][1], acc[c][2], acc[c][3], floor2);
            om[planar_at(0, oy, ox, OW, OH)] = (uint8_t)q;
            om[planar_at(1, oy, ox, OW, OH)] = (uint8_t)(q >> 8);
            om[planar_at(2, oy, ox, OW, OH)] = (uint8_t)(q >> 16);
        } else {
            if (my >= IH || mx >= IW) continue;
            const uint32_t q = pack4_relu7(acc[c][0], acc[c][1], acc[c][2], acc[c][3], floor2);
            uint8_t *op = om + ((size_t)(2 * my + (g >> 1)) * OW + (2 * mx + (g & 1))) * 3;
            op[0] = (uint8_t)q;
            op[1] = (uint8_t)(q >> 8);
            op[2] = (uint8_t)(q >> 16);
        }
    }
}

}  // namespace sicn
