// The tile body of the channel-generic MFMA kernels: one 16 x 16 tile of M positions x one block of 64 output channels of ONE image
// (and, for the deconv, one phase).  k_any (k_mfma16c.hip: equal-size batches, the image is blockIdx.z) and k_any_ragged
// (k_ragged.hip: images of different sizes, the image comes from a table) differ only in how a workgroup finds its image and its
// tile; from there on both run any_tile().  The layout of the patch, of the weight image and of the accumulators is described at
// the head of k_mfma16c.hip.
#pragma once
#include "k_common.hpp"

namespace sicn {

constexpr int ANY_T = 16;                        // tile edge in M positions
constexpr int ANY_CONV_EDGE = 2 * ANY_T + 3;     // 35 input pixels
constexpr int ANY_DECONV_EDGE = ANY_T + 2;       // 18
constexpr int ANY_MAX_CH = 1024;

__host__ __device__ constexpr int any_patch_pixels(bool deconv) { return deconv ? ANY_DECONV_EDGE * ANY_DECONV_EDGE : ANY_CONV_EDGE * ANY_CONV_EDGE; }
__host__ __device__ constexpr size_t any_lds_bytes(bool deconv) { return (size_t)any_patch_pixels(deconv) * 64; }

// conv parity plane (a, b) = (row & 1, column & 1) of the 35 x 35 patch: (18 - a) rows of (18 - b) pixels, planes back to back
__device__ __forceinline__ int any_plane_base(int a, int b) { return a * (18 * 18 + 18 * 17) + b * (a ? 17 * 18 : 18 * 18); }
__device__ __forceinline__ int any_plane_pitch(int b) { return 18 - b; }

// im / om: the image's own [IH][IW][C] input and [OH][OW][O] output; (y0, x0): the tile's origin in M positions; (qy, qx): the
// deconv phase; J: the block of 64 output channels; smem: any_lds_bytes(DECONV) bytes
template <bool DECONV, int NT>
__device__ __forceinline__ void any_tile(const uint8_t *__restrict__ im, uint8_t *__restrict__ om, const int8_t *__restrict__ wimg,
                                         const int8_t *__restrict__ bias, int IW, int IH, int C, int OW, int OH, int O, int y0, int x0,
                                         int qy, int qx, int J, uint32_t floor2, uint8_t *smem)
{
    constexpr int EDGE = DECONV ? ANY_DECONV_EDGE : ANY_CONV_EDGE;
    constexpr int UNITS = EDGE * EDGE * 4;                     // 16-byte units of one chunk's patch
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int nchunk = (C + 63) >> 6;
    const bool rgb_in = C == 3;
    const int iy0 = DECONV ? y0 - 1 : 2 * y0 - 2, ix0 = DECONV ? x0 - 1 : 2 * x0 - 2;   // input pixel of patch pixel (0, 0)

    // accumulators start from the bias
    v4i acc[4][NT];
#pragma unroll
    for (int j = 0; j < NT; j++) {
        v4i b;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int o = NT == 4 ? 64 * J + 16 * g + 4 * j + r : 4 * g + r;
            b[r] = o < O ? (int)bias[o] : 0;
        }
#pragma unroll
        for (int c = 0; c < 4; c++) acc[c][j] = b;
    }

    const int ntap = DECONV ? (3 - qy) * (3 - qx) : 25;
    for (int n = 0; n < nchunk; n++) {
        if (n) __syncthreads();                                 // every wave is done with the previous chunk's patch
        // ---- stage the patch of chunk n: 16-byte units, four loads in flight per thread
#pragma unroll 1
        for (int u0 = 0; u0 < UNITS; u0 += 4 * 256) {
            uint4 v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int u = u0 + i * 256 + tid;
                v[i] = uint4{0u, 0u, 0u, 0u};
                if (u < UNITS) {
                    const int pp = u >> 2, c0 = n * 64 + 16 * (u & 3);
                    const int pr = pp / EDGE, pc = pp - pr * EDGE;
                    const int iy = iy0 + pr, ix = ix0 + pc;
                    if (iy >= 0 && iy < IH && ix >= 0 && ix < IW && c0 < C) {
                        const uint8_t *s = im + ((size_t)iy * IW + ix) * C + c0;
                        if (rgb_in)
                            v[i].x = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16;
                        else                                    // C % 16 == 0: the unit is all inside the pixel
                            v[i] = *reinterpret_cast<const uint4 *>(s);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int u = u0 + i * 256 + tid;
                if (u < UNITS) {
                    const int pp = u >> 2;
                    const int pr = pp / EDGE, pc = pp - pr * EDGE;
                    const int slot = DECONV ? pp : any_plane_base(pr & 1, pc & 1) + (pr >> 1) * any_plane_pitch(pc & 1) + (pc >> 1);
                    *reinterpret_cast<uint4 *>(smem + (size_t)slot * 64 + 16 * (u & 3)) = v[i];
                }
            }
        }
        __syncthreads();

        // ---- the taps of this chunk
        auto request = [&](int t, v4i(&bf)[4], v4i(&af)[NT]) {
            int ky, kx, slot, pitch;
            if (DECONV) {
                const int nx = 3 - qx, iy = t / nx, ix = t - iy * nx;
                ky = 2 * iy + qy;
                kx = 2 * ix + qx;
                pitch = ANY_DECONV_EDGE;                        // patch pixel of position (ly, lx): (ly + qy + iy, lx + qx + ix)
                slot = (4 * wv + qy + iy) * pitch + col + qx + ix;
            } else {
                ky = t / 5;
                kx = t - ky * 5;
                pitch = any_plane_pitch(kx & 1);                // patch pixel (2 ly + ky, 2 lx + kx) -> plane (ky & 1, kx & 1)
                slot = any_plane_base(ky & 1, kx & 1) + (4 * wv + (ky >> 1)) * pitch + col + (kx >> 1);
            }
#pragma unroll
            for (int c = 0; c < 4; c++) bf[c] = *reinterpret_cast<const v4i *>(smem + (size_t)(slot + c * pitch) * 64 + 16 * g);
            const int8_t *wt = wimg + ((((size_t)J * 25 + (ky * 5 + kx)) * nchunk + n) * NT) * 1024 + col * 64 + 16 * g;
#pragma unroll
            for (int j = 0; j < NT; j++) af[j] = *reinterpret_cast<const v4i *>(wt + j * 1024);
        };
        auto multiply = [&](const v4i(&bf)[4], const v4i(&af)[NT]) {
#pragma unroll
            for (int j = 0; j < NT; j++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[c][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[j], bf[c], acc[c][j], 0, 0, 0);
        };
        v4i bf0[4], af0[NT], bf1[4], af1[NT];
        request(0, bf0, af0);
#pragma unroll 1
        for (int t = 0; t < ntap; t += 2) {
            if (t + 1 < ntap) request(t + 1, bf1, af1);
            multiply(bf0, af0);
            if (t + 1 < ntap) {
                if (t + 2 < ntap) request(t + 2, bf0, af0);
                multiply(bf1, af1);
            }
        }
    }

    // ---- epilogue: one truncation mod 256, then relu7 or the raw byte (floor2), straight from the accumulators
    const int MW = DECONV ? IW : OW, MH = DECONV ? IH : OH;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int my = y0 + 4 * wv + c, mx = x0 + col;
        if (my >= MH || mx >= MW) continue;
        const int oy = DECONV ? 2 * my + qy : my, ox = DECONV ? 2 * mx + qx : mx;
        uint8_t *op = om + ((size_t)oy * OW + ox) * O;
        if constexpr (NT == 4) {
            const int o0 = 64 * J + 16 * g;
            if (o0 >= O) continue;                              // OFM_CH % 16 == 0: the lane's 16 channels are all real or all padding
            uint4 q;
            q.x = pack4_relu7(acc[c][0][0], acc[c][0][1], acc[c][0][2], acc[c][0][3], floor2);
            q.y = pack4_relu7(acc[c][1][0], acc[c][1][1], acc[c][1][2], acc[c][1][3], floor2);
            q.z = pack4_relu7(acc[c][2][0], acc[c][2][1], acc[c][2][2], acc[c][2][3], floor2);
            q.w = pack4_relu7(acc[c][3][0], acc[c][3][1], acc[c][3][2], acc[c][3][3], floor2);
            *reinterpret_cast<uint4 *>(op + o0) = q;
        } else if (g == 0) {                                  // natural rows: C/D rows 0 .. 2 are the RGB channels
            const uint32_t q = pack4_relu7(acc[c][0][0], acc[c][0][1], acc[c][0][2], acc[c][0][3], floor2);
#pragma unroll
            for (int r = 0; r < 3; r++)
                if (r < O) op[r] = (uint8_t)(q >> (8 * r));
        }
    }
}

}  // namespace sicn
