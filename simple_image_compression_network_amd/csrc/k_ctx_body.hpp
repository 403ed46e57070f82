// Container mode 4, "rANS-WC": the device code of the context coder, shared by the uniform batch kernels (sicn_codec_ctx.inc:
// blockIdx.y = image, every image of one shape, pointers advancing by uniform strides) and the ragged ones (k_ragged_ctx.hip: flat
// grids over the work items of n images of n shapes, each image found through a table).  Every stage is a __device__ function of ONE
// image's pointers, its CtxGeom and the index of the work item INSIDE the image (a chunk of dwords, a group of streams).
// The pointers pass through `at`, which names the three address spaces a stage touches — at.lat(p): the latent / scale tensors,
// at.ws(p): the workspace, at.slot(p): the slot buffer — and turns a pointer into THIS image's.  The uniform kernels hand in image
// 0's pointers and CtxStrided (+ blockIdx.y * stride, applied where a pointer is first used: their instructions are those of the
// kernels that held this text before it moved here, profiles/ragged_ctx_resource_usage.txt); the ragged kernels resolve their image
// before the call and hand in CtxResolved.  The format: oracle/sicn_hyper_oracle.c.
#pragma once
#include <type_traits>

#include "k_codec_body.hpp"

namespace {

constexpr int NCLS = 16;
constexpr uint32_t CTX_TABLE_BYTES = NCLS * 256;   // in the container: 16 x 128 x u16

struct CtxGeom {
    uint32_t W, H, C, nsym[2], nst[2];
};
__host__ __device__ inline CtxGeom ctx_geom(uint32_t W, uint32_t H, uint32_t C)
{
    const uint32_t a = (W + 1) / 2, b = W / 2;
    CtxGeom g;
    g.W = W; g.H = H; g.C = C;
    g.nsym[0] = ((H / 2) * W + ((H & 1) ? a : 0)) * C;
    g.nsym[1] = ((H / 2) * W + ((H & 1) ? b : 0)) * C;
    g.nst[0] = (g.nsym[0] + WSS - 1) / WSS;
    g.nst[1] = (g.nsym[1] + WSS - 1) / WSS;
    return g;
}

// pixel j of a set (0 = anchors: (x + y) even, 1 = non-anchors), raster order inside the set
__device__ __forceinline__ void ctx_pixel(int set, uint32_t j, uint32_t W, uint32_t &y, uint32_t &x)
{
    const uint32_t a = (W + 1) / 2, b = W / 2, r = j / W, t = j - r * W;
    if (set == 0) {
        if (t < a) { y = 2 * r; x = 2 * t; } else { y = 2 * r + 1; x = 2 * (t - a) + 1; }
    } else {
        if (t < b) { y = 2 * r; x = 2 * t + 1; } else { y = 2 * r + 1; x = 2 * (t - b); }
    }
}

// byte-wise max of two dwords whose bytes are all < 128
__device__ __forceinline__ uint32_t max4_u7(uint32_t a, uint32_t b)
{
    const uint32_t d = (a | 0x80808080u) - b;                 // no borrow between bytes; bit 7 of a byte set iff a >= b there
    const uint32_t m = ((d >> 7) & 0x01010101u) * 0xFFu;
    return (a & m) | (b & ~m);
}

// classes (one per byte) of the 4 consecutive channels at byte offset `off` = ((y W + x) C + ch) of latent / scale
__device__ __forceinline__ uint32_t ctx_class4(int set, const uint8_t *lat, const uint8_t *scale, uint32_t W, uint32_t H, uint32_t C,
                                               uint32_t y, uint32_t x, uint32_t off)
{
    const uint32_t k0 = (*reinterpret_cast<const uint32_t *>(scale + off) >> 3) & 0x0F0F0F0Fu;   // s < 128
    if (set == 0) return k0;
    uint32_t m = 0;
    if (y > 0) m = max4_u7(m, *reinterpret_cast<const uint32_t *>(lat + off - W * C) & 0x7F7F7F7Fu);
    if (y + 1 < H) m = max4_u7(m, *reinterpret_cast<const uint32_t *>(lat + off + W * C) & 0x7F7F7F7Fu);
    if (x > 0) m = max4_u7(m, *reinterpret_cast<const uint32_t *>(lat + off - C) & 0x7F7F7F7Fu);
    if (x + 1 < W) m = max4_u7(m, *reinterpret_cast<const uint32_t *>(lat + off + C) & 0x7F7F7F7Fu);
    return ((k0 + ((m >> 3) & 0x0F0F0F0Fu) + 0x01010101u) >> 1) & 0x0F0F0F0Fu;   // bytes <= 31 before the shift: no carries
}

struct CtxWorkspace {        // per image, carved out of the caller's workspace
    uint32_t *hist;          // [256] + sums (64 B) + freq (256 B, unused) + meta (64 B): the block k_clear_stats zeroes
    unsigned long long *sums;
    uint32_t *meta;          // [0] error flags, [1] payload bytes the streams may use, [2] header adler32, [3] stream errors
    uint32_t *chist;         // [16][128] class histograms
    uint32_t *tfc;           // [16][128] freq | cum << 16
    uint32_t *trcp;          // [16][128] reciprocals (encoder)
    uint8_t *tst;            // [16][4096] slot -> symbol (decoder; round 3: [16][256], the first symbol of every 16-slot bucket + a search)
    uint32_t *lens, *offsets;
    uint8_t *scratch;
};
__host__ __device__ inline size_t ctx_carve(CtxWorkspace &w, void *base, uint32_t ns, size_t scratch_per_stream)
{
    uint8_t *p = (uint8_t *)base;
    size_t off = 0;
    w.hist = (uint32_t *)(p + off); off += 1024;
    w.sums = (unsigned long long *)(p + off); off += 64;
    off += 256;
    w.meta = (uint32_t *)(p + off); off += 64;
    w.chist = (uint32_t *)(p + off); off += NCLS * 128 * 4;
    w.tfc = (uint32_t *)(p + off); off += NCLS * 128 * 4;
    w.trcp = (uint32_t *)(p + off); off += NCLS * 128 * 4;
    w.tst = p + off; off += NCLS * 4096;
    w.lens = (uint32_t *)(p + off); off += align_up(4 * (size_t)ns + 4, 64);
    w.offsets = (uint32_t *)(p + off); off += align_up(4 * (size_t)ns + 4, 64);
    w.scratch = p + off;
    off += (size_t)ns * scratch_per_stream;
    return off;
}
// `at` of a stage whose pointers are already this image's (k_ragged_ctx.hip)
struct CtxResolved {
    template <typename T> __device__ __forceinline__ T *lat(T *p) const { return p; }
    template <typename T> __device__ __forceinline__ T *ws(T *p) const { return p; }
    template <typename T> __device__ __forceinline__ T *slot(T *p) const { return p; }
};
inline size_t ctx_ws_bytes(uint32_t ns) { CtxWorkspace w; return align_up(ctx_carve(w, nullptr, ns, WCAP) + 64, 256); }
// workgroups of the class-histogram stage that share one image of n symbols
inline uint32_t ctx_hist_blocks(uint32_t n) { const uint32_t b = (n / 4 + 255u) / 256u; return b < 256u ? b : 256u; }

// class histograms (+ range check of the scale map); one thread per dword of 4 channels.  Workgroup `bx` of the `nb` that share the image.
template <class At>
__device__ __forceinline__ void ctx_hist_body(const At &at, const uint8_t *lat_, const uint8_t *scale_, const CtxGeom &g, uint32_t *chist_,
                                              uint32_t *meta_, uint32_t bx, uint32_t nb)
{
    const uint8_t *lat = at.lat(lat_), *scale = at.lat(scale_);
    uint32_t *chist = at.ws(chist_), *meta = at.ws(meta_);
    __shared__ uint32_t h[NCLS * 128];
    for (int i = threadIdx.x; i < NCLS * 128; i += 256) h[i] = 0;
    __syncthreads();
    const uint32_t ndw = g.W * g.H * g.C / 4, cdw = g.C / 4;
    bool bad = false;
    for (uint32_t i = bx * 256 + threadIdx.x; i < ndw; i += nb * 256) {
        const uint32_t px = i / cdw, y = px / g.W, x = px - y * g.W, off = 4 * i;
        const uint32_t v = *reinterpret_cast<const uint32_t *>(lat + off);
        bad |= ((v | *reinterpret_cast<const uint32_t *>(scale + off)) & 0x80808080u) != 0;
        const uint32_t k4 = ctx_class4((int)((x + y) & 1u), lat, scale, g.W, g.H, g.C, y, x, off);
#pragma unroll
        for (int b = 0; b < 4; b++) atomicAdd(&h[((k4 >> (8 * b)) & 15u) * 128 + ((v >> (8 * b)) & 127u)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NCLS * 128; i += 256)
        if (h[i]) atomicAdd(&chist[i], h[i]);
    if (bad) atomicOr(&meta[0], 1u);
}

// 16 waves, one per class: histogram -> 12-bit table (the walk of k_enc_header), container bytes, and the encoder's /
// decoder's lookup images.  Wave 0 also writes the header.
// encoder: table_in_ == nullptr, tables come from chist and go to out_; decoder: tables are READ from the container
template <class At>
__device__ __forceinline__ void ctx_tables_body(const At &at, const uint32_t *chist_, const unsigned long long *sums_, uint32_t *meta_,
                                                uint32_t *tfc_, uint32_t *trcp_, uint8_t *tst_, uint8_t *out_, const CtxGeom &g,
                                                uint32_t img_w, uint32_t img_h, const uint8_t *table_in_)
{
    const int lane = threadIdx.x & 63, cls = threadIdx.x >> 6;
    uint32_t *meta = at.ws(meta_), *tfc = at.ws(tfc_) + cls * 128, *trcp = at.ws(trcp_) + cls * 128;
    uint8_t *tst = at.ws(tst_) + cls * 4096;
    uint32_t f[2], err = 0;
    if (table_in_) {
        const uint8_t *t = at.slot(table_in_) + cls * 256 + 4 * lane;
        const bool readable = (meta[0] & 0x100u) == 0;
        f[0] = readable ? (t[0] | ((uint32_t)t[1] << 8)) : 0u;
        f[1] = readable ? (t[2] | ((uint32_t)t[3] << 8)) : 0u;
        int sum = (int)(f[0] + f[1]);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        if (sum != 0 && sum != 4096) { err = 8; f[0] = f[1] = 0; }
    } else {
        const uint32_t *hist = at.ws(chist_) + cls * 128;
        const uint32_t h0 = hist[2 * lane], h1 = hist[2 * lane + 1];
        uint32_t n = h0 + h1;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) n += (uint32_t)__shfl_xor((int)n, d);
        const uint32_t hh[2] = {h0, h1};
#pragma unroll
        for (int k = 0; k < 2; k++) {
            unsigned long long v = (hh[k] && n) ? ((unsigned long long)hh[k] * 4096u) / n : 0;
            if (hh[k] && v == 0) v = 1;
            f[k] = (uint32_t)v;
        }
        int sum = (int)(f[0] + f[1]);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        int diff = n ? 4096 - sum : 0;
        for (int it = 0; it < 200 && diff != 0; it++) {
            uint32_t key = 0;
#pragma unroll
            for (int k = 0; k < 2; k++)
                if (f[k] > 0 && (diff > 0 || f[k] > 1)) key = max(key, (f[k] << 8) | (uint32_t)(255 - (2 * lane + k)));
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, d));
            if (key == 0) break;
            const int best = 255 - (int)(key & 255u), fb = (int)(key >> 8);
            const int step = diff > 0 ? diff : (diff < 1 - fb ? 1 - fb : diff);
            if ((best >> 1) == lane) f[best & 1] = (uint32_t)(fb + step);
            diff -= step;
        }
        if (diff != 0) { err = 2; f[0] = f[1] = 0; }
        uint8_t *ft = at.slot(out_) + SICN_CODEC_HEADER_BYTES + cls * 256 + 4 * lane;
        ft[0] = (uint8_t)f[0]; ft[1] = (uint8_t)(f[0] >> 8); ft[2] = (uint8_t)f[1]; ft[3] = (uint8_t)(f[1] >> 8);
    }
    // exclusive prefix sums -> freq | cum << 16, reciprocals, bucket table
    uint32_t incl = f[0] + f[1];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= d) incl += up;
    }
    const uint32_t c0 = incl - f[0] - f[1], c1 = c0 + f[0];
    tfc[2 * lane] = f[0] | (c0 << 16);
    tfc[2 * lane + 1] = f[1] | (c1 << 16);
    trcp[2 * lane] = ransw_rcp(f[0]);
    trcp[2 * lane + 1] = ransw_rcp(f[1]);
    if (table_in_) {   // decoder only: slot -> symbol, 4096 slots per class.  Lane l fills slots 64 l .. 64 l + 63: a binary search for the
        // first one, then a walk along the cumulative table (filling "my symbol's range" instead left one lane with most of a
        // peaked table: 38 us per image set)
        __shared__ uint16_t cum[NCLS][130];
        cum[cls][2 * lane] = (uint16_t)c0;
        cum[cls][2 * lane + 1] = (uint16_t)c1;
        if (lane == 63) cum[cls][128] = 0xFFFFu;   // sentinel: the walk stops at symbol 127
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint16_t *cm = cum[cls];
        const uint32_t v0 = 64u * (uint32_t)lane;
        uint32_t lo = 0, hi = 128;                 // largest sy with cm[sy] <= v0 (cm[0] = 0): a zero-frequency run ends at the symbol that owns the slot
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cm[mid] <= v0) lo = mid; else hi = mid;
        }
        uint32_t sy = lo, nb = cm[sy + 1];
        uint32_t outw[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            uint32_t wv4 = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t v = v0 + 4u * (uint32_t)i + (uint32_t)b;
                while (v >= nb) { sy++; nb = cm[sy + 1]; }
                wv4 |= sy << (8 * b);
            }
            outw[i] = wv4;
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
            *reinterpret_cast<uint4 *>(tst + v0 + 16 * i) = make_uint4(outw[4 * i], outw[4 * i + 1], outw[4 * i + 2], outw[4 * i + 3]);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) err |= (uint32_t)__shfl_xor((int)err, d);
    if (lane == 0 && err) atomicOr(&meta[0], err);
    if (!table_in_ && threadIdx.x < 12) {   // header (dword 10 = payload bytes comes from the scan)
        const unsigned long long *sums = at.ws(sums_);
        const uint32_t n = g.W * g.H * g.C;
        const uint32_t a = (uint32_t)((1 + sums[0]) % ADLER_MOD), b = (uint32_t)((n % ADLER_MOD + sums[1]) % ADLER_MOD);
        const uint32_t words[12] = {0x4C434953u, 1u | (4u << 16), img_w, img_h, g.W, g.H, g.C, n, g.nst[0] + g.nst[1], WSS, 0u, (b << 16) | a};
        if (threadIdx.x != 10) {
            const uint32_t v = words[threadIdx.x];
            uint8_t *p = at.slot(out_) + 4 * threadIdx.x;
            p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
        }
    }
}

// the error word of an image's statistics / table stages (after every stage has run), by ONE lane
__device__ __forceinline__ uint32_t ctx_enc_verdict(const uint32_t *meta, const uint32_t *hist)
{
    uint32_t err = meta[0];
    for (int s = 128; s < 256; s++)
        if (hist[s]) err |= 1u;
    return err;
}

// Round 4: FOUR streams (waves) per workgroup share one copy of the class tables.  A one-wave workgroup carried 16 + 8 KB of LDS
// (12 + 8 in the decoder): six / eight waves per CU — 1.5 / 2 per SIMD — for step loops that are chains of dependent LDS
// round trips.  Shared, the tables cost 4 / 3 KB per wave and twelve waves fit.  A ring is private to its wave and a wave's LDS
// operations execute in order, so the flush / fill points (data-dependent, different in every wave) need no block barrier — only
// the compiler has to keep the order (wave_lds_sync).
constexpr uint32_t CTX_WPB = 4;
// what k_ctx_encode_steps.inc / k_ctx_decode_steps.inc check of the names their including kernel must have declared
template <class Name, class Want> constexpr bool ctx_names = std::is_same_v<std::remove_cv_t<std::remove_reference_t<Name>>, Want>;
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one set per launch (anchors first): CTX_WPB_DEC streams of the set per workgroup.  The symbol of a slot comes from ONE table read
// (16 classes x 4096 slots = 64 KB of LDS, shared by the workgroup's eight waves; round 3 read the first symbol of a 16-slot
// bucket and walked the cumulative table from there — up to a dozen dependent LDS round trips per step on a flat class, with
// six waves per CU to hide them behind).  The step loops themselves: k_ctx_encode_steps.inc, k_ctx_decode_steps.inc.
constexpr uint32_t CTX_WPB_DEC = 8;

// header of a mode-4 container `c` against the caller's shape (the tables are checked by the tables stage), by one wave.
// `valid`: bytes of the slot that may be read.  Clears the image's statistics block: the first stage of a decode.
template <class At>
__device__ __forceinline__ void ctx_parse_body(const At &at, const uint8_t *containers_, uint32_t valid, uint32_t *meta_, const CtxGeom &g)
{
    const uint8_t *c = at.slot(containers_);
    uint32_t *meta = at.ws(meta_);
    const int lane = threadIdx.x;
    const uint32_t ns = g.nst[0] + g.nst[1], n = g.W * g.H * g.C;
    const size_t fixed = SICN_CODEC_HEADER_BYTES + CTX_TABLE_BYTES + 4 * (size_t)ns;
    clear_stats_in_parse(meta, lane);
    if (valid < fixed) {
        if (lane == 0) { meta[0] = 0x104u; meta[1] = 0; meta[2] = 0; meta[3] = 0; }
        return;
    }
    auto rd32 = [&](int o) { return c[o] | ((uint32_t)c[o + 1] << 8) | ((uint32_t)c[o + 2] << 16) | ((uint32_t)c[o + 3] << 24); };
    const uint32_t expect[10] = {0x4C434953u, 1u | (4u << 16), 0, 0, g.W, g.H, g.C, n, ns, WSS};
    uint32_t err = 0;
    if (lane < 10 && lane != 2 && lane != 3 && rd32(4 * lane) != expect[lane]) err = 4;
    const uint32_t pb = rd32(40);
    if ((size_t)pb > (size_t)valid - fixed) err |= 16;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) err |= (uint32_t)__shfl_xor((int)err, d);
    if (lane == 0) {
        meta[0] = err;
        meta[1] = (err & 16) ? 0u : pb;
        meta[2] = rd32(44);
        meta[3] = 0;
    }
}

}  // namespace
