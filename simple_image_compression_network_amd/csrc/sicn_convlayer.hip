// Generic finn-hlslib ConvLayer_Batch surface (include/sicn_convlayer.h): any kernel size, channel
// count, fold, accumulator width, pass-through or multi-threshold activation, 1- / 2- / 4- / 8-bit input lanes, 2- to 32-bit output lanes:
//   acc  = wrap_TA( sum_{ky,kx,c} x[y+ky][x+kx][c] * W[o][(ky*K+kx)*C + c] )      mvau.hpp:87-179
//   out  = low OUT_BIT bits of  activation(acc)                                    activations.hpp:127-190
// Stride 1, no padding, square image (convlayer.h:116-118).  Parity unpinned (no reference outputs
// exist for this surface, sicn_convlayer.h).
//
// Three kernels.  k_convlayer_patch (every descriptor): implicit GEMM on v_mfma_i32_16x16x64_i8 with the input patch of a 16 x 16 output
// tile unpacked into LDS (int8 lanes padded to 64 channels, double-buffered), the output lanes packed in the epilogue.
// k_convlayer_mfma (IN_BIT 8, OUT_BIT >= 8, IFM_CH a multiple of 16 — where it measured faster): a wave owns 64 consecutive
// output positions x 64 output channels (16 accumulator tiles); a K step is 64 channel bytes of ONE kernel tap, read straight from the
// NHWC image (16 bytes per lane, the cache hierarchy serves the K*K-fold reuse).  Both take the weights from a zero-padded
// [O/16][tap][C/64][16][64] image; int8 x int8 is signed x signed: 8-bit unsigned inputs are read as x - 128 (one v_xor per dword) and
// 128 * sum_k W[o][k] is the accumulators' start value.  k_convlayer: one thread per output byte or container, direct evaluation — the
// cross-check (SICN_CONVLAYER_KERNEL_DIRECT).  None is a tuned hot path (that is sicn.h).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <new>
#include <vector>

#include "../../include/sicn.h"
#include "../../include/sicn_convlayer.h"
#include "sicn_weights_io.h"

struct sicn_convlayer_params {
    sicn_convlayer_desc d;
    int8_t *d_w_okc;     // [OFM_CH][K*K*IFM_CH] sign-extended weights
    int32_t *d_thr;      // [OFM_CH][NUM_TH] thresholds in channel order, or nullptr
    int8_t *d_w_mfma;    // [ceil(O/16)][K*K][ceil(C/64)][16 rows][64 bytes], zero padded
    int32_t *d_wsum;     // [ceil(O/16)*16] sum_k W[o][k]
};

namespace {

__device__ __forceinline__ long long wrap_acc(long long v, int bits, int is_signed)
{
    const unsigned long long mask = bits >= 64 ? ~0ull : ((1ull << bits) - 1);
    unsigned long long u = (unsigned long long)v & mask;
    if (is_signed && bits < 64 && (u >> (bits - 1)) & 1) return (long long)(u | ~mask);
    return (long long)u;
}

// lane c of a pixel's stream word (interpret.hpp:191-244: Slice<ap_(u)int<W>> reads bits [c W, (c + 1) W)), W in {1, 2, 4, 8}: never
// straddles a byte
__device__ __forceinline__ int lane_value(const uint8_t *pixel, int c, int bits, int is_signed)
{
    const int off = c * bits;
    int v = (pixel[off >> 3] >> (off & 7)) & ((1 << bits) - 1);
    if (is_signed && (v >> (bits - 1))) v -= 1 << bits;
    return v;
}

// one thread per output UNIT: a byte holding 8 / OUT_BIT lanes (OUT_BIT < 8) or one lane's container (OUT_BIT >= 8)
__global__ __launch_bounds__(256) void k_convlayer(const uint8_t *__restrict__ in, void *__restrict__ out,
                                                   const int8_t *__restrict__ w_okc, const int32_t *__restrict__ thr,
                                                   sicn_convlayer_desc d)
{
    const int lanes_per_unit = d.OUT_BIT < 8 ? 8 / d.OUT_BIT : 1;
    const int units_per_pixel = d.OFM_CH / lanes_per_unit;
    const size_t per_img = (size_t)d.OFM_DIM * d.OFM_DIM * units_per_pixel;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per_img) return;
    const int img = blockIdx.y;
    const int unit = (int)(idx % units_per_pixel);
    const size_t pix = idx / units_per_pixel;
    const int x = (int)(pix % d.OFM_DIM), y = (int)(pix / d.OFM_DIM);
    const int C = d.IFM_CH, K = d.K;
    const int in_pixel_bytes = C * d.IN_BIT / 8;
    const uint8_t *im = in + (size_t)img * d.IFM_DIM * d.IFM_DIM * in_pixel_bytes;
    uint32_t packed = 0;
    for (int l = 0; l < lanes_per_unit; l++) {
        const int o = unit * lanes_per_unit + l;
        const int8_t *wo = w_okc + (size_t)o * K * K * C;
        long long acc = 0;   // exact: |sum| <= 121 * C * 255 * 128 fits easily
        for (int ky = 0; ky < K; ky++)
            for (int kx = 0; kx < K; kx++) {
                const uint8_t *s = im + ((size_t)(y + ky) * d.IFM_DIM + (x + kx)) * in_pixel_bytes;
                const int8_t *wk = wo + (ky * K + kx) * C;
                if (d.IN_BIT == 8) {
                    if (d.IN_SIGNED)
                        for (int c = 0; c < C; c++) acc += (int)(int8_t)s[c] * (int)wk[c];
                    else
                        for (int c = 0; c < C; c++) acc += (int)s[c] * (int)wk[c];
                } else
                    for (int c = 0; c < C; c++) acc += lane_value(s, c, d.IN_BIT, d.IN_SIGNED) * (int)wk[c];
            }
        const long long a = wrap_acc(acc, d.ACC_BIT, d.ACC_SIGNED);   // TA: every += wraps, the final wrap is the same
        long long r = a;
        if (d.activation == SICN_ACT_THRESHOLDS) {
            r = d.ACT_VAL;
            const int32_t *t = thr + (size_t)o * d.NUM_TH;
            for (int i = 0; i < d.NUM_TH; i++) r += (wrap_acc((long long)t[i], d.ACC_BIT, d.ACC_SIGNED) < a) ? 1 : 0;
        }
        if (d.OUT_BIT < 8)
            packed |= ((uint32_t)r & ((1u << d.OUT_BIT) - 1)) << (l * d.OUT_BIT);   // lane o in bits [o OUT_BIT, (o + 1) OUT_BIT) of the word
        else
            packed = (uint32_t)r;
    }
    const size_t oi = (size_t)img * per_img + idx;
    if (d.OUT_BIT <= 8)
        ((uint8_t *)out)[oi] = (uint8_t)packed;
    else if (d.OUT_BIT == 16)
        ((uint16_t *)out)[oi] = (uint16_t)packed;
    else
        ((uint32_t *)out)[oi] = packed;
}

typedef int v4i_t __attribute__((ext_vector_type(4)));

// wave = 64 consecutive output positions (4 column tiles of 16) x 64 output channels (4 weight tiles)
__global__ __launch_bounds__(256) void k_convlayer_mfma(const uint8_t *__restrict__ in, void *__restrict__ out,
                                                        const int8_t *__restrict__ wm, const int32_t *__restrict__ wsum,
                                                        const int32_t *__restrict__ thr, sicn_convlayer_desc d)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int C = d.IFM_CH, K = d.K, D = d.IFM_DIM, OD = d.OFM_DIM, O = d.OFM_CH;
    const int npos = OD * OD, nchunk = (C + 63) / 64, KK = K * K;
    const int p0 = (blockIdx.x * 4 + wv) * 64;            // first position of this wave
    const int j0 = blockIdx.y * 4;                        // first 16-channel weight tile
    const int ntile = (O + 15) / 16;
    const uint8_t *img = in + (size_t)blockIdx.z * D * D * C;
    if (p0 >= npos) return;

    // this lane's pixel (per column tile): top-left corner of its window, as a byte offset
    uint32_t pix[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        int p = p0 + 16 * c + col;
        p = p < npos ? p : npos - 1;                      // clamped positions are computed and not stored
        const int y = p / OD, x = p - y * OD;
        pix[c] = (uint32_t)((y * D + x) * C);
    }
    v4i_t acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v4i_t b;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int o = (j0 + j) * 16 + 4 * g + r;       // C/D row 4g + r of tile j
            b[r] = (d.IN_SIGNED || j0 + j >= ntile) ? 0 : 128 * wsum[o];
        }
#pragma unroll
        for (int c = 0; c < 4; c++) acc[c][j] = b;
    }
    const uint32_t flip = d.IN_SIGNED ? 0u : 0x80808080u;
    // K walk: step s = (tap t, 64-channel chunk cc), t outer.  The operands of step s + 1 are requested before the 16 MFMAs of step s
    // (round 5: the loop used to load, wait and multiply — one exposed memory round trip per step; two register sets, the loop unrolled by two)
    const int nstep = KK * nchunk;
    int t_n = 0, cc_n = 0, ky_n = 0, kx_n = 0;            // the step the next request is for
    auto request = [&](v4i_t (&bf)[4], v4i_t (&af)[4]) {
        const uint32_t tap = (uint32_t)((ky_n * D + kx_n) * C);
        const int c0 = cc_n * 64 + 16 * g;                // this lane's 16 channel bytes of the K step
        const bool valid = c0 < C;                         // C % 16 == 0: a 16-byte group is all in or all out (weights 0)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint4 q = *reinterpret_cast<const uint4 *>(img + pix[c] + tap + (valid ? c0 : 0));
            bf[c] = v4i_t{(int)(q.x ^ flip), (int)(q.y ^ flip), (int)(q.z ^ flip), (int)(q.w ^ flip)};
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int jj = j0 + j < ntile ? j0 + j : ntile - 1;
            af[j] = *reinterpret_cast<const v4i_t *>(wm + ((((size_t)jj * KK + t_n) * nchunk + cc_n) * 16 + col) * 64 + 16 * g);
        }
        if (++cc_n == nchunk) {
            cc_n = 0;
            t_n++;
            if (++kx_n == K) {
                kx_n = 0;
                ky_n++;
            }
        }
    };
    auto multiply = [&](const v4i_t (&bf)[4], const v4i_t (&af)[4]) {
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[c][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[j], bf[c], acc[c][j], 0, 0, 0);
    };
    v4i_t bf0[4], af0[4], bf1[4], af1[4];
    request(bf0, af0);
    for (int s_ = 0; s_ < nstep; s_ += 2) {
        if (s_ + 1 < nstep) request(bf1, af1);
        multiply(bf0, af0);
        if (s_ + 1 < nstep) {
            if (s_ + 2 < nstep) request(bf0, af0);
            multiply(bf1, af1);
        }
    }
    // epilogue: lane holds, per (column tile c, weight tile j), channels 16(j0+j) + 4g .. +3 of position p0 + 16c + col
    const size_t per_img = (size_t)npos * O;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int p = p0 + 16 * c + col;
        if (p >= npos) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = (j0 + j) * 16 + 4 * g + r;
                if (o >= O) continue;
                const long long a = wrap_acc((long long)acc[c][j][r], d.ACC_BIT, d.ACC_SIGNED);
                long long res = a;
                if (d.activation == SICN_ACT_THRESHOLDS) {
                    res = d.ACT_VAL;
                    const int32_t *tt = thr + (size_t)o * d.NUM_TH;
                    for (int i = 0; i < d.NUM_TH; i++) res += (wrap_acc((long long)tt[i], d.ACC_BIT, d.ACC_SIGNED) < a) ? 1 : 0;
                }
                const size_t oi = (size_t)blockIdx.z * per_img + (size_t)p * O + o;
                if (d.OUT_BIT == 8)
                    ((uint8_t *)out)[oi] = (uint8_t)res;
                else if (d.OUT_BIT == 16)
                    ((uint16_t *)out)[oi] = (uint16_t)res;
                else
                    ((uint32_t *)out)[oi] = (uint32_t)res;
            }
        }
    }
}

// ---- k_convlayer_patch: every descriptor, any IN_BIT / OUT_BIT / IFM_CH / OFM_CH (LDS-staged implicit GEMM) ----------------------------
// A workgroup = a PT x PT tile of output positions of one image x 64 output channels (blockIdx.y); wave wv owns tile rows 4 wv .. 4 wv + 3,
// one 16-position column tile per row.  K walk: 64-channel chunks outside, the K x K taps inside.  For each chunk the input patch of
// (PT + K - 1)^2 pixels sits in LDS as 64 int8 lanes per pixel (64 bytes), 0 for channels >= IFM_CH and pixels outside the image; the
// B operand of tap (ky, kx) is 16 lanes of the patch pixel (row + ky, col + kx), the A operand comes from the weight image as in
// k_convlayer_mfma.  The patch is double-buffered: the next chunk is staged in pieces of PIECE dwords per thread, a piece's global loads
// issued before one tap's MFMAs and its LDS writes after them.
constexpr int PT = 16;      // output tile edge (positions)
constexpr int PIECE = 4;    // patch dwords per thread per staging piece

__host__ __device__ constexpr int patch_edge(int K) { return PT + K - 1; }
__host__ __device__ constexpr size_t patch_lds_bytes(int K) { return 2 * (size_t)patch_edge(K) * patch_edge(K) * 64; }   // two buffers

// Patch dword u of chunk n = lanes n*64 + 4q .. +3 (q = u & 15) of patch pixel u >> 4.  The stream is read as aligned dwords (a pixel can be
// 1, 2 or 3 bytes): the nl * IN_BIT bits of the unit start at bit `bit` of the batch, in the dword that holds it and, when they cross into
// it, the next one.  Both hold stream bits, so a load never leaves the aligned dwords of the buffer.
struct PatchUnit {
    uint32_t lo, hi, meta;   // meta = shift | nbits << 8; nbits 0: a zero dword (padding channel or a pixel outside the image)
};

__device__ __forceinline__ PatchUnit patch_request(const uint32_t *__restrict__ base32, uint64_t img_bit0, int u, int n, int y0, int x0, int PW,
                                                   const sicn_convlayer_desc &d)
{
    PatchUnit r{0u, 0u, 0u};
    const int pp = u >> 4, c = n * 64 + 4 * (u & 15);   // pp < PW * PW
    const int pr = pp / PW, pc = pp - pr * PW;
    const int y = y0 + pr, x = x0 + pc;
    if (y < d.IFM_DIM && x < d.IFM_DIM && c < d.IFM_CH) {
        const int nb = (d.IFM_CH - c < 4 ? d.IFM_CH - c : 4) * d.IN_BIT;
        const uint64_t bit = img_bit0 + ((uint64_t)(y * d.IFM_DIM + x) * d.IFM_CH + c) * d.IN_BIT;
        const uint32_t sh = (uint32_t)bit & 31;
        r.lo = base32[bit >> 5];
        if (sh + nb > 32) r.hi = base32[(bit >> 5) + 1];
        r.meta = sh | (uint32_t)nb << 8;
    }
    return r;
}

// the unit's lanes as 4 int8 (byte i = lane i): ap_int lanes sign-extended, ap_uint sub-byte lanes as they are, 8-bit ap_uint lanes as
// x - 128 (k_convlayer_mfma's convention); lanes past IFM_CH are 0
__device__ __forceinline__ uint32_t patch_lanes(const PatchUnit &r, int in_bit, int in_signed)
{
    const int sh = r.meta & 255, nb = r.meta >> 8;
    if (nb == 0) return 0u;
    const uint64_t v = ((((uint64_t)r.hi << 32) | r.lo) >> sh) & ((1ull << nb) - 1);
    if (in_bit == 8) return (uint32_t)v ^ (in_signed ? 0u : 0x80808080u & (uint32_t)((1ull << nb) - 1));
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int l = (int)(v >> (i * in_bit)) & ((1 << in_bit) - 1);
        if (in_signed) l = (int)((uint32_t)l << (32 - in_bit)) >> (32 - in_bit);
        out |= ((uint32_t)l & 255u) << (8 * i);
    }
    return out;   // lanes past nb read as 0 bits: 0
}

__global__ __launch_bounds__(256) void k_convlayer_patch(const uint8_t *__restrict__ in, void *__restrict__ out,
                                                         const int8_t *__restrict__ wm, const int32_t *__restrict__ wsum,
                                                         const int32_t *__restrict__ thr, sicn_convlayer_desc d)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int C = d.IFM_CH, K = d.K, D = d.IFM_DIM, OD = d.OFM_DIM, O = d.OFM_CH;
    const int PW = patch_edge(K), KK = K * K, nchunk = (C + 63) / 64, ntile = (O + 15) / 16;
    const int tiles_x = (OD + PT - 1) / PT;
    const int y0 = (int)(blockIdx.x / tiles_x) * PT, x0 = (int)(blockIdx.x % tiles_x) * PT;
    const int j0 = blockIdx.y * 4;                                   // first 16-channel weight tile
    const int nt = ntile - j0 < 4 ? ntile - j0 : 4;                  // weight tiles of this workgroup (uniform)
    const int img = blockIdx.z;
    const size_t buf_bytes = (size_t)PW * PW * 64;
    const int units = PW * PW * 16, npieces = (units + 256 * PIECE - 1) / (256 * PIECE);

    const uint32_t *base32 = reinterpret_cast<const uint32_t *>((uintptr_t)in & ~(uintptr_t)3);
    const uint64_t img_bit0 = ((uintptr_t)in & 3) * 8 + (uint64_t)img * D * D * C * d.IN_BIT;

    // one piece of chunk n: PIECE dwords per thread, requested, then written to buffer `dst`
    auto piece_request = [&](PatchUnit (&pu)[PIECE], int piece, int n) {
#pragma unroll
        for (int i = 0; i < PIECE; i++) {
            const int u = (piece * PIECE + i) * 256 + tid;
            pu[i] = u < units ? patch_request(base32, img_bit0, u, n, y0, x0, PW, d) : PatchUnit{0u, 0u, 0u};
        }
    };
    auto piece_write = [&](const PatchUnit (&pu)[PIECE], int piece, uint8_t *dst) {
#pragma unroll
        for (int i = 0; i < PIECE; i++) {
            const int u = (piece * PIECE + i) * 256 + tid;
            if (u < units) reinterpret_cast<uint32_t *>(dst)[u] = patch_lanes(pu[i], d.IN_BIT, d.IN_SIGNED);
        }
    };

    v4i_t acc[4][4];
    const bool bias = !d.IN_SIGNED && d.IN_BIT == 8;                // x - 128 lanes: 128 * sum_k W[o][k] to start with
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v4i_t b;
#pragma unroll
        for (int r = 0; r < 4; r++) b[r] = (bias && j < nt) ? 128 * wsum[(j0 + j) * 16 + 4 * g + r] : 0;
#pragma unroll
        for (int c = 0; c < 4; c++) acc[c][j] = b;
    }

    for (int piece = 0; piece < npieces; piece++) {                   // chunk 0 into buffer 0
        PatchUnit pu[PIECE];
        piece_request(pu, piece, 0);
        piece_write(pu, piece, smem);
    }
    __syncthreads();

    for (int n = 0; n < nchunk; n++) {
        const uint8_t *cur = smem + (n & 1) * buf_bytes;
        uint8_t *nxt = smem + ((n + 1) & 1) * buf_bytes;
        const bool stage = n + 1 < nchunk;
        int piece = 0;
        // B of tap t: 16 lanes (16 g ..) of patch pixel (4 wv + c + ky, col + kx); A: the weight image's 16 x 64 block (tile, tap, chunk)
        auto request = [&](int t, v4i_t (&bf)[4], v4i_t (&af)[4]) {
            const int ky = t / K, kx = t - ky * K;
#pragma unroll
            for (int c = 0; c < 4; c++)
                bf[c] = *reinterpret_cast<const v4i_t *>(cur + ((size_t)(4 * wv + c + ky) * PW + col + kx) * 64 + 16 * g);
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (j < nt) af[j] = *reinterpret_cast<const v4i_t *>(wm + ((((size_t)(j0 + j) * KK + t) * nchunk + n) * 16 + col) * 64 + 16 * g);
        };
        auto multiply = [&](const v4i_t (&bf)[4], const v4i_t (&af)[4]) {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (j < nt)
#pragma unroll
                    for (int c = 0; c < 4; c++) acc[c][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[j], bf[c], acc[c][j], 0, 0, 0);
        };
        // one tap: the next piece's loads go out before the MFMAs, its LDS writes follow them
        auto tap = [&](const v4i_t (&bf)[4], const v4i_t (&af)[4]) {
            const bool go = stage && piece < npieces;                   // uniform
            PatchUnit pu[PIECE];
            if (go) piece_request(pu, piece, n + 1);
            multiply(bf, af);
            if (go) piece_write(pu, piece++, nxt);
        };
        v4i_t bf0[4], af0[4], bf1[4], af1[4];
        request(0, bf0, af0);
        for (int t = 0; t < KK; t += 2) {
            if (t + 1 < KK) request(t + 1, bf1, af1);
            tap(bf0, af0);
            if (t + 1 < KK) {
                if (t + 2 < KK) request(t + 2, bf0, af0);
                tap(bf1, af1);
            }
        }
        for (; stage && piece < npieces; piece++) {                    // what the taps did not cover (K <= 2)
            PatchUnit pu[PIECE];
            piece_request(pu, piece, n + 1);
            piece_write(pu, piece, nxt);
        }
        __syncthreads();
    }

    // epilogue: lane holds, per (tile row c, weight tile j), channels 16 (j0 + j) + 4 g .. + 3 of position (y0 + 4 wv + c, x0 + col)
    const int word_units = d.OUT_BIT < 8 ? O * d.OUT_BIT / 8 : O;     // bytes (OUT_BIT 2 / 4) or containers per pixel
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int oy = y0 + 4 * wv + c, ox = x0 + col;
        if (oy >= OD || ox >= OD) continue;
        const size_t pix = ((size_t)img * OD + oy) * OD + ox;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j >= nt) continue;
            uint32_t res[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = (j0 + j) * 16 + 4 * g + r;
                const long long a = wrap_acc((long long)acc[c][j][r], d.ACC_BIT, d.ACC_SIGNED);
                long long v = a;
                if (d.activation == SICN_ACT_THRESHOLDS) {
                    v = d.ACT_VAL;
                    if (o < O) {
                        const int32_t *tt = thr + (size_t)o * d.NUM_TH;
                        for (int i = 0; i < d.NUM_TH; i++) v += (wrap_acc((long long)tt[i], d.ACC_BIT, d.ACC_SIGNED) < a) ? 1 : 0;
                    }
                }
                res[r] = (uint32_t)v;
            }
            const int o0 = (j0 + j) * 16 + 4 * g;
            uint8_t *ob = (uint8_t *)out + pix * word_units;
            if (d.OUT_BIT == 2) {                                       // lanes o0 .. o0 + 3 = byte o0 / 4 of the pixel word
                if (o0 / 4 < word_units)
                    ob[o0 / 4] = (uint8_t)((res[0] & 3) | (res[1] & 3) << 2 | (res[2] & 3) << 4 | (res[3] & 3) << 6);
            } else if (d.OUT_BIT == 4) {                                // bytes o0 / 2 and o0 / 2 + 1
                if (o0 / 2 < word_units) ob[o0 / 2] = (uint8_t)((res[0] & 15) | (res[1] & 15) << 4);
                if (o0 / 2 + 1 < word_units) ob[o0 / 2 + 1] = (uint8_t)((res[2] & 15) | (res[3] & 15) << 4);
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    if (o0 + r >= O) continue;
                    if (d.OUT_BIT == 8)
                        ob[o0 + r] = (uint8_t)res[r];
                    else if (d.OUT_BIT == 16)
                        ((uint16_t *)out)[pix * O + o0 + r] = (uint16_t)res[r];
                    else
                        ((uint32_t *)out)[pix * O + o0 + r] = res[r];
                }
            }
        }
    }
}

}  // namespace

extern "C" int sicn_convlayer_validate(const sicn_convlayer_desc *d)
{
    if (!d) return SICN_EINVAL;
    if (d->K < 1 || d->K > 11 || d->IFM_CH <= 0 || d->OFM_CH <= 0 || d->SIMD <= 0 || d->PE <= 0) return SICN_EINVAL;
    if (d->IFM_DIM < d->K || d->IFM_DIM > (1 << 15) || d->OFM_DIM != d->IFM_DIM - d->K + 1) return SICN_EINVAL;
    if (d->IFM_CH % d->SIMD || d->OFM_CH % d->PE) return SICN_EINVAL;   // slidingwindow.h:177, mvau.hpp:101-105
    if ((d->IN_BIT != 1 && d->IN_BIT != 2 && d->IN_BIT != 4 && d->IN_BIT != 8) || (d->IN_SIGNED != 0 && d->IN_SIGNED != 1)) return SICN_EINVAL;
    if ((d->IFM_CH * d->IN_BIT) % 8) return SICN_EINVAL;   // a pixel's stream word is whole bytes
    if (d->W_BIT < 2 || d->W_BIT > 8 || d->SIMD * d->W_BIT > 64) return SICN_EINVAL;
    if ((long long)d->W_TILES != (long long)(d->OFM_CH / d->PE) * ((long long)d->K * d->K * d->IFM_CH / d->SIMD)) return SICN_EINVAL;
    if (d->ACC_BIT < 1 || d->ACC_BIT > 32 || (d->ACC_SIGNED != 0 && d->ACC_SIGNED != 1)) return SICN_EINVAL;
    if (d->OUT_BIT != 2 && d->OUT_BIT != 4 && d->OUT_BIT != 8 && d->OUT_BIT != 16 && d->OUT_BIT != 32) return SICN_EINVAL;
    if ((d->OFM_CH * d->OUT_BIT) % 8) return SICN_EINVAL;
    if (d->activation == SICN_ACT_PASSTHROUGH) {
        if (d->NUM_TH != 0) return SICN_EINVAL;
    } else if (d->activation == SICN_ACT_THRESHOLDS) {
        if (d->NUM_TH < 1 || d->NUM_TH > 1024) return SICN_EINVAL;
    } else
        return SICN_EINVAL;
    return SICN_OK;
}

namespace {
enum ConvLayerKernel { CL_DIRECT, CL_MFMA, CL_PATCH };

// what SICN_CONVLAYER_KERNEL_AUTO launches for a valid descriptor.  Byte lanes in, containers out and IFM_CH % 16 == 0 stay on
// k_convlayer_mfma: it measured faster than k_convlayer_patch on every such shape timed
ConvLayerKernel pick_kernel(const sicn_convlayer_desc &d)
{
    if ((size_t)d.IFM_DIM * d.IFM_DIM * d.IFM_CH >= 0x7fffffffu) return CL_DIRECT;   // 31-bit per-image lane offsets
    if (d.IN_BIT == 8 && d.OUT_BIT >= 8 && d.IFM_CH % 16 == 0) return CL_MFMA;
    return CL_PATCH;
}
}  // namespace

extern "C" const char *sicn_convlayer_kernel_for(const sicn_convlayer_desc *d)
{
    if (sicn_convlayer_validate(d)) return nullptr;
    switch (pick_kernel(*d)) {
    case CL_MFMA: return "k_convlayer_mfma";
    case CL_PATCH: return "k_convlayer_patch";
    default: return "k_convlayer";
    }
}

extern "C" void sicn_convlayer_params_free(sicn_convlayer_params *p)
{
    if (!p) return;
    if (p->d_w_okc) (void)hipFree(p->d_w_okc);
    if (p->d_thr) (void)hipFree(p->d_thr);
    if (p->d_w_mfma) (void)hipFree(p->d_w_mfma);
    if (p->d_wsum) (void)hipFree(p->d_wsum);
    delete p;
}

extern "C" int sicn_convlayer_params_create(const sicn_convlayer_desc *d, const void *m_weights, int word_bytes,
                                            const int32_t *thresholds, sicn_convlayer_params **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    int rc = sicn_convlayer_validate(d);
    if (rc) return rc;
    if (!m_weights || (word_bytes != 1 && word_bytes != 2 && word_bytes != 4 && word_bytes != 8)) return SICN_EINVAL;
    if (d->SIMD * d->W_BIT > word_bytes * 8) return SICN_EINVAL;
    if ((d->activation == SICN_ACT_THRESHOLDS) != (thresholds != nullptr)) return SICN_EINVAL;
    const int kk = d->K * d->K * d->IFM_CH, nf_n = d->OFM_CH / d->PE;
    std::vector<int8_t> w;
    std::vector<int32_t> t;
    try {
        w.resize((size_t)d->OFM_CH * kk);
        if (thresholds) t.resize((size_t)d->OFM_CH * d->NUM_TH);
    } catch (const std::bad_alloc &) { return SICN_ENOMEM; }
    sicn::decode_finn_tiles(m_weights, word_bytes, d->W_BIT, d->SIMD, d->PE, d->W_TILES, kk, d->OFM_CH, w.data());
    if (thresholds)   // ThresholdsActivation::m_thresholds[PE][NF][NumTH] -> [o][i]
        for (int pe = 0; pe < d->PE; pe++)
            for (int nf = 0; nf < nf_n; nf++)
                for (int i = 0; i < d->NUM_TH; i++)
                    t[(size_t)(nf * d->PE + pe) * d->NUM_TH + i] = thresholds[((size_t)pe * nf_n + nf) * d->NUM_TH + i];
    sicn_convlayer_params *p = new (std::nothrow) sicn_convlayer_params();
    if (!p) return SICN_ENOMEM;
    p->d = *d;
    p->d_w_okc = nullptr;
    p->d_thr = nullptr;
    p->d_w_mfma = nullptr;
    p->d_wsum = nullptr;
    bool ok = sicn::upload(w.data(), w.size(), &p->d_w_okc);
    if (ok) {   // the MFMA image: [O/16][tap][C/64][16 rows][64 bytes], zero padded
        const int KK = d->K * d->K, nchunk = (d->IFM_CH + 63) / 64, ntile = (d->OFM_CH + 15) / 16;
        std::vector<int8_t> wm;
        std::vector<int32_t> ws;
        try {
            wm.assign((size_t)ntile * KK * nchunk * 16 * 64, 0);
            ws.assign((size_t)ntile * 16, 0);
        } catch (const std::bad_alloc &) {
            sicn_convlayer_params_free(p);
            return SICN_ENOMEM;
        }
        for (int o = 0; o < d->OFM_CH; o++)
            for (int t = 0; t < KK; t++)
                for (int c = 0; c < d->IFM_CH; c++) {
                    const int8_t v = w[(size_t)o * kk + t * d->IFM_CH + c];
                    wm[((((size_t)(o / 16) * KK + t) * nchunk + c / 64) * 16 + o % 16) * 64 + c % 64] = v;
                    ws[o] += v;
                }
        ok = sicn::upload(wm.data(), wm.size(), &p->d_w_mfma) && sicn::upload(ws.data(), ws.size() * 4, &p->d_wsum);
    }
    if (ok && thresholds) ok = sicn::upload(t.data(), t.size() * 4, &p->d_thr);
    if (!ok) {
        sicn_convlayer_params_free(p);
        return SICN_ENOMEM;
    }
    *out = p;
    return SICN_OK;
}

extern "C" int sicn_conv_layer_batch(const sicn_convlayer_desc *d, const sicn_convlayer_params *p, const uint8_t *in,
                                     void *out, int reps, void *hip_stream)
{
    return sicn_conv_layer_batch_kernel(d, p, in, out, reps, SICN_CONVLAYER_KERNEL_AUTO, hip_stream);
}

extern "C" int sicn_conv_layer_batch_kernel(const sicn_convlayer_desc *d, const sicn_convlayer_params *p, const uint8_t *in,
                                            void *out, int reps, int kernel, void *hip_stream)
{
    if (kernel != SICN_CONVLAYER_KERNEL_AUTO && kernel != SICN_CONVLAYER_KERNEL_DIRECT) return SICN_EINVAL;
    int rc = sicn_convlayer_validate(d);
    if (rc) return rc;
    if (!p || !in || !out || reps < 0 || reps > 65535) return SICN_EINVAL;
    const sicn_convlayer_desc &q = p->d;   // the parameters must have been made for this layer
    if (q.K != d->K || q.IFM_CH != d->IFM_CH || q.OFM_CH != d->OFM_CH || q.W_BIT != d->W_BIT ||
        q.activation != d->activation || q.NUM_TH != d->NUM_TH)
        return SICN_EINVAL;
    if (reps == 0) return SICN_OK;
    if (q.IN_BIT != d->IN_BIT || q.IN_SIGNED != d->IN_SIGNED) return SICN_EINVAL;
    const size_t per_img = (size_t)d->OFM_DIM * d->OFM_DIM * (d->OUT_BIT < 8 ? d->OFM_CH * d->OUT_BIT / 8 : d->OFM_CH);   // output units
    const size_t blocks = (per_img + 255) / 256;
    if (blocks > 0x7fffffffu) return SICN_EINVAL;
    const ConvLayerKernel k = kernel == SICN_CONVLAYER_KERNEL_DIRECT ? CL_DIRECT : pick_kernel(*d);
    if (k == CL_MFMA) {
        const unsigned npos = (unsigned)(d->OFM_DIM * d->OFM_DIM);
        dim3 grid((npos + 255) / 256, (unsigned)((d->OFM_CH + 63) / 64), (unsigned)reps);
        hipLaunchKernelGGL(k_convlayer_mfma, grid, dim3(256), 0, (hipStream_t)hip_stream, in, out, p->d_w_mfma, p->d_wsum,
                           p->d_thr, *d);
        return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
    }
    if (k == CL_PATCH) {
        const unsigned tiles_x = (unsigned)((d->OFM_DIM + PT - 1) / PT);
        dim3 grid(tiles_x * tiles_x, (unsigned)((d->OFM_CH + 63) / 64), (unsigned)reps);
        const size_t lds = patch_lds_bytes(d->K);
        if (hipFuncSetAttribute((const void *)k_convlayer_patch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return SICN_ENODEV;
        hipLaunchKernelGGL(k_convlayer_patch, grid, dim3(256), lds, (hipStream_t)hip_stream, in, out, p->d_w_mfma, p->d_wsum, p->d_thr, *d);
        return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
    }
    hipLaunchKernelGGL(k_convlayer, dim3((unsigned)blocks, (unsigned)reps), dim3(256), 0, (hipStream_t)hip_stream, in, out,
                       p->d_w_okc, p->d_thr, *d);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}
