// Container mode 4, "rANS-WC": the device code of the context coder, shared by the uniform batch kernels (sicn_codec_ctx.inc:
// blockIdx.y = image, every image of one shape, pointers advancing by uniform strides) and the ragged ones (k_ragged_ctx.hip: flat
// grids over the work items of n images of n shapes, each image found through a table).  Every stage is a __device__ function of ONE
// image (CtxImage: its geometry, latent, scale map, container slot and workspace block, already resolved to pointers) and of the index
// of the work item INSIDE the image (a chunk of dwords, a group of streams).  Both kinds of kernel name an image by one CtxRow and
// turn it into that context with ctx_image(); they differ only in where the row comes from (CtxBatch: computed; ragged: loaded) —
// the shape k_codec_body.hpp gives mode 3.  The format: oracle/sicn_hyper_oracle.c.
#pragma once
#include "k_codec_body.hpp"

// include/sicn_ctx_stream_length.h (declared here so that the uniform coder's translation unit does not see the ragged ABI)
extern "C" size_t sicn_codec_ctx_max_bytes_sl(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t stream_symbols);

namespace {

constexpr int NCLS = 16;
constexpr uint32_t CTX_TABLE_BYTES = NCLS * 256;   // in the container: 16 x 128 x u16

// S: the stream length, header dword 9 (wstream_ok: a power of two, 1024 .. 16384).  Each set is cut into streams of S symbols; a
// stream's scratch slot and the bound of its length entry are wstream_cap(S) bytes.  It belongs to the image: the uniform entry
// points give every image of a batch one S, the ragged coder keeps one per row.
struct CtxGeom {
    uint32_t W, H, C, nsym[2], nst[2], S;
};
__host__ __device__ inline CtxGeom ctx_geom(uint32_t W, uint32_t H, uint32_t C, uint32_t S)
{
    const uint32_t a = (W + 1) / 2, b = W / 2;
    CtxGeom g;
    g.W = W; g.H = H; g.C = C;
    g.nsym[0] = ((H / 2) * W + ((H & 1) ? a : 0)) * C;
    g.nsym[1] = ((H / 2) * W + ((H & 1) ? b : 0)) * C;
    g.S = S;
    g.nst[0] = (g.nsym[0] + S - 1) / S;
    g.nst[1] = (g.nsym[1] + S - 1) / S;
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
    uint32_t *hist;          // [256] + sums (64 B) + freq (256 B, unused) + meta (64 B): the statistics block, cleared before a coding
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
// host: what ctx_carve says about a block without a block: the byte offset of the class histograms (carved from address 0), the size
inline size_t ctx_chist_offset() { CtxWorkspace w; ctx_carve(w, nullptr, 0, 0); return reinterpret_cast<uintptr_t>(w.chist); }
inline size_t ctx_ws_bytes(uint32_t ns, uint32_t S) { CtxWorkspace w; return align_up(ctx_carve(w, nullptr, ns, wstream_cap(S)) + 64, 256); }
// workgroups of the class-histogram stage that share one image of n symbols
inline uint32_t ctx_hist_blocks(uint32_t n) { const uint32_t b = (n / 4 + 255u) / 256u; return b < 256u ? b : 256u; }

// ---- one image as the kernels name it -------------------------------------------------------------------------------------
// Geometry and 64-bit byte offsets into the latent / scale tensors, the slot buffer and the workspace; the workspace block of an image
// is what ctx_carve() gives for its stream count.  The ragged coder keeps a table of these (k_ragged_ctx.hip).
struct CtxRow {
    uint64_t lat_off, slot_off, ws_off;
    CtxGeom g;
    uint32_t slot_cap;                 // min(slot bytes, 2^32 - 1): nothing of a slot is read beyond it
    uint32_t img_w, img_h;
    uint32_t first_chunk, n_chunks;    // ragged: the image's first work items in the flat grids; n_chunks: its statistics workgroups
    uint32_t first_enc, first_dec[2], first_stream;
};
inline uint32_t ctx_slot_cap(uint64_t slot_bytes) { return (uint32_t)(slot_bytes < 0xFFFFFFFFull ? slot_bytes : 0xFFFFFFFFull); }
// host: the fields of a row that follow from the image's shape (slot_cap: that of the smallest slot the ragged layout gives, a caller
// with slots of its own overwrites it), and the shape limits of both families of entry points.  32-bit stream offsets: the scratch
// slots of all streams, wstream_cap(S) bytes each, must stay below 2^32 (mode 3's rule, sicn_codec.hip wstream_fits) — at 16384
// MAX_RANS_SYMBOLS implies it, at 1024 it is the tighter limit (about 1.9 G symbols).
inline int ctx_row_shape(CtxRow &r, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t img_w, uint32_t img_h, uint32_t S)
{
    const uint64_t positions = (uint64_t)lat_w * lat_h;
    if (positions == 0 || lat_c == 0 || (lat_c & 3) || !wstream_ok(S)) return SICN_EINVAL;
    if (positions > MAX_RANS_SYMBOLS || positions * lat_c > MAX_RANS_SYMBOLS) return SICN_EINVAL;   // (the products cannot wrap)
    r.g = ctx_geom(lat_w, lat_h, lat_c, S);
    if (((uint64_t)r.g.nst[0] + r.g.nst[1]) * wstream_cap(S) >= (1ull << 32)) return SICN_EINVAL;
    r.slot_cap = ctx_slot_cap(align_up(sicn_codec_ctx_max_bytes_sl(lat_w, lat_h, lat_c, S), 16));
    r.img_w = img_w; r.img_h = img_h;
    r.n_chunks = ctx_hist_blocks((uint32_t)(positions * lat_c));
    return SICN_OK;
}
// a row of a table in memory (the ragged kernels), every field wave-uniform
__device__ __forceinline__ CtxRow load_row(const CtxRow *__restrict__ rows, uint32_t img)
{
    const CtxRow *r = rows + img;
    return CtxRow{uni(r->lat_off), uni(r->slot_off), uni(r->ws_off),
                  CtxGeom{uni(r->g.W), uni(r->g.H), uni(r->g.C), {uni(r->g.nsym[0]), uni(r->g.nsym[1])}, {uni(r->g.nst[0]), uni(r->g.nst[1])}, uni(r->g.S)},
                  uni(r->slot_cap), uni(r->img_w), uni(r->img_h), uni(r->first_chunk), uni(r->n_chunks), uni(r->first_enc),
                  {uni(r->first_dec[0]), uni(r->first_dec[1])}, uni(r->first_stream)};
}
// A uniform batch (sicn_codec_ctx.inc: blockIdx.y = image, every image of one shape) is image 0's row (offsets 0: the kernels get the
// base pointers) and three byte strides.  Passed by value, so it lives in kernel-argument SGPRs.
struct CtxBatch {
    CtxRow row0;
    uint64_t s_lat, s_slot, s_ws;
};
__device__ __forceinline__ CtxRow batch_row(const CtxBatch &b)
{
    CtxRow r = b.row0;
    r.lat_off += blockIdx.y * b.s_lat; r.slot_off += blockIdx.y * b.s_slot; r.ws_off += blockIdx.y * b.s_ws;
    return r;
}

// ---- one image as the stages see it ---------------------------------------------------------------------------------------
// One type for both directions: the encoder reads `lat` and writes `slot`, the decoder the reverse, so both are writable here.
struct CtxImage {
    CtxGeom g;
    uint8_t *lat;                  // [H][W][C] symbols
    const uint8_t *scale;          // [H][W][C] the hyper-synthesis scale map
    uint8_t *slot;                 // container slot: header, class tables, length table, payload
    uint32_t slot_cap;
    uint32_t img_w, img_h;
    CtxWorkspace w;
};
__device__ __forceinline__ CtxImage ctx_image(const CtxRow &r, const uint8_t *latents, const uint8_t *scales, const uint8_t *containers,
                                              uint8_t *workspace)
{
    CtxImage im;
    im.g = r.g;
    im.lat = const_cast<uint8_t *>(latents) + r.lat_off;
    im.scale = scales + r.lat_off;
    im.slot = const_cast<uint8_t *>(containers) + r.slot_off;
    im.slot_cap = r.slot_cap;
    im.img_w = r.img_w; im.img_h = r.img_h;
    ctx_carve(im.w, workspace + r.ws_off, r.g.nst[0] + r.g.nst[1], wstream_cap(r.g.S));
    return im;
}

// ---- stages ---------------------------------------------------------------------------------------------------------------
// class histograms (+ range check of the scale map); one thread per dword of 4 channels.  Workgroup `bx` of the `nb` that share the image.
__device__ __forceinline__ void ctx_hist_body(const CtxImage &im, uint32_t bx, uint32_t nb)
{
    const CtxGeom &g = im.g;
    const uint8_t *lat = im.lat, *scale = im.scale;
    uint32_t *chist = im.w.chist, *meta = im.w.meta;
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

// 16 waves, one per class: histogram -> 12-bit table (the walk of normalize_wave), container bytes, and the encoder's /
// decoder's lookup images.  Wave 0 also writes the header.
// encoder (!dec): the tables come from the class histograms and go to the container; decoder: they are READ from the container
__device__ __forceinline__ void ctx_tables_body(const CtxImage &im, bool dec)
{
    const CtxGeom &g = im.g;
    const int lane = threadIdx.x & 63, cls = threadIdx.x >> 6;
    uint32_t *meta = im.w.meta, *tfc = im.w.tfc + cls * 128, *trcp = im.w.trcp + cls * 128;
    uint8_t *tst = im.w.tst + cls * 4096;
    uint32_t f[2], err = 0;
    if (dec) {
        const uint8_t *t = im.slot + SICN_CODEC_HEADER_BYTES + cls * 256 + 4 * lane;
        const bool readable = (meta[0] & 0x100u) == 0;
        f[0] = readable ? (t[0] | ((uint32_t)t[1] << 8)) : 0u;
        f[1] = readable ? (t[2] | ((uint32_t)t[3] << 8)) : 0u;
        int sum = (int)(f[0] + f[1]);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        if (sum != 0 && sum != 4096) { err = 8; f[0] = f[1] = 0; }
    } else {
        const uint32_t *hist = im.w.chist + cls * 128;
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
        uint8_t *ft = im.slot + SICN_CODEC_HEADER_BYTES + cls * 256 + 4 * lane;
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
    if (dec) {   // decoder only: slot -> symbol, 4096 slots per class.  Lane l fills slots 64 l .. 64 l + 63: a binary search for the
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
    if (!dec && threadIdx.x < 12) {   // header (dword 10 = payload bytes comes from the scan)
        const unsigned long long *sums = im.w.sums;
        const uint32_t n = g.W * g.H * g.C;
        const uint32_t a = (uint32_t)((1 + sums[0]) % ADLER_MOD), b = (uint32_t)((n % ADLER_MOD + sums[1]) % ADLER_MOD);
        const uint32_t words[12] = {0x4C434953u, 1u | (4u << 16), im.img_w, im.img_h, g.W, g.H, g.C, n, g.nst[0] + g.nst[1], g.S, 0u, (b << 16) | a};
        if (threadIdx.x != 10) {
            const uint32_t v = words[threadIdx.x];
            uint8_t *p = im.slot + 4 * threadIdx.x;
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

// header of a mode-4 container against the caller's shape (the tables are checked by the tables stage), by one wave.  `valid`: a
// sicn_codec_status array whose .bytes bound the slots (entry `img` is this image's), or nullptr = slot_cap.  Clears the image's
// statistics block: the first stage of a decode.
__device__ __forceinline__ void ctx_parse_body(const CtxImage &im, const uint32_t *valid_, uint32_t img)
{
    const CtxGeom &g = im.g;
    const uint8_t *c = im.slot;
    uint32_t *meta = im.w.meta;
    const uint32_t valid = valid_ ? min(valid_[2 * (size_t)img + 1], im.slot_cap) : im.slot_cap;   // sicn_codec_status.bytes
    const int lane = threadIdx.x;
    const uint32_t ns = g.nst[0] + g.nst[1], n = g.W * g.H * g.C;
    const size_t fixed = SICN_CODEC_HEADER_BYTES + CTX_TABLE_BYTES + 4 * (size_t)ns;
    clear_stats_in_parse(meta, lane);
    if (valid < fixed) {
        if (lane == 0) { meta[0] = 0x104u; meta[1] = 0; meta[2] = 0; meta[3] = 0; }
        return;
    }
    auto rd32 = [&](int o) { return c[o] | ((uint32_t)c[o + 1] << 8) | ((uint32_t)c[o + 2] << 16) | ((uint32_t)c[o + 3] << 24); };
    const uint32_t expect[10] = {0x4C434953u, 1u | (4u << 16), 0, 0, g.W, g.H, g.C, n, ns, g.S};
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

// Round 4: FOUR streams (waves) per workgroup share one copy of the class tables.  A one-wave workgroup carried 16 + 8 KB of LDS
// (12 + 8 in the decoder): six / eight waves per CU — 1.5 / 2 per SIMD — for step loops that are chains of dependent LDS
// round trips.  Shared, the tables cost 4 / 3 KB per wave and twelve waves fit.  A ring is private to its wave and a wave's LDS
// operations execute in order, so the flush / fill points (data-dependent, different in every wave) need no block barrier — only
// the compiler has to keep the order (wave_lds_sync).
constexpr uint32_t CTX_WPB = 4;
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// encoder: group `grp` of CTX_WPB streams of the image, anchors and non-anchors numbered through
__device__ __forceinline__ void ctx_encode_body(const CtxImage &im, uint32_t grp)
{
    const CtxGeom &g = im.g;
    const uint8_t *lat = im.lat, *scale = im.scale;
    const uint32_t *tfc = im.w.tfc, *trcp = im.w.trcp;
    uint8_t *scratch = im.w.scratch;
    uint32_t *lens = im.w.lens;
    __shared__ uint32_t fc[NCLS * 128], rcp[NCLS * 128];
    __shared__ __attribute__((aligned(16))) uint16_t words_all[CTX_WPB][RING_WORDS];   // one ring per wave, see ransw_encode_body
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, st = grp * CTX_WPB + wv;
    for (uint32_t i = threadIdx.x; i < NCLS * 128; i += 64 * CTX_WPB) { fc[i] = tfc[i]; rcp[i] = trcp[i]; }
    __syncthreads();
    if (st >= g.nst[0] + g.nst[1]) return;   // (no block barrier below this line)
    uint16_t *words = words_all[wv];
    const int set = st >= g.nst[0];
    const uint32_t q0 = set ? st - g.nst[0] : st;
    const uint32_t begin = q0 * g.S, cnt = min(g.S, g.nsym[set] - begin), blocks = (cnt + 255) / 256, cap = wstream_cap(g.S);
    uint16_t *dst = (uint16_t *)(scratch + (size_t)st * cap);
    uint32_t pos = cap / 2, top = cap / 2, x = RANSW_L;
    const unsigned long long below = (1ull << lane) - 1;
    auto load = [&](uint32_t q, uint32_t &sym4, uint32_t &cls4) {   // C % 4 == 0: a lane's 4 symbols are 4 channels of one pixel
        const uint32_t j = q * 256 + lane * 4;
        sym4 = cls4 = 0;
        if (j >= cnt) return;
        const uint32_t e = begin + j, px = e / g.C, ch = e - px * g.C;
        uint32_t y, xx;
        ctx_pixel(set, px, g.W, y, xx);
        const uint32_t off = (y * g.W + xx) * g.C + ch;
        sym4 = *reinterpret_cast<const uint32_t *>(lat + off);
        cls4 = ctx_class4(set, lat, scale, g.W, g.H, g.C, y, xx, off);
    };
    uint32_t nsym = 0, ncls = 0;
    if (blocks) load(blocks - 1, nsym, ncls);
    for (uint32_t q = blocks; q-- > 0;) {
        const uint32_t sym4 = nsym, cls4 = ncls;
        if (q) load(q - 1, nsym, ncls);
#pragma unroll
        for (int k = 3; k >= 0; k--) {
            const bool active0 = q * 256 + lane * 4 + k < cnt;
            const uint32_t idx = ((cls4 >> (8 * k)) & 15u) * 128 + ((sym4 >> (8 * k)) & 127u);
            const uint32_t t = fc[idx], c = t >> 16;
            uint32_t f = t & 0xFFFFu;
            const bool active = active0 && f != 0;      // f == 0 only for input the statistics stage rejected
            f = active ? f : 1u;
            const bool emit = active && (unsigned long long)x >= ((unsigned long long)f << 20);
            const unsigned long long mask = __ballot(emit);
            pos -= (uint32_t)__popcll(mask);
            if (emit) {
                words[(pos + (uint32_t)__popcll(mask & below)) & (RING_WORDS - 1)] = (uint16_t)x;
                x >>= 16;
            }
            if (active) {
                uint32_t r;
                const uint32_t qq = ransw_div(x, f, rcp[idx], r);
                x = (qq << PROB_BITS) + r + c;
            }
        }
        if (top - pos > RING_WORDS - 4 * 64 - 128) {
            wave_lds_sync();
            ring_flush(words, dst, pos, top, lane);
            wave_lds_sync();
            top = pos;
        }
    }
    pos -= 128;
    words[(pos + 2 * lane) & (RING_WORDS - 1)] = (uint16_t)x;
    words[(pos + 2 * lane + 1) & (RING_WORDS - 1)] = (uint16_t)(x >> 16);
    wave_lds_sync();
    ring_flush(words, dst, pos, top, lane);
    if (lane == 0) lens[st] = (cap / 2 - pos) * 2;
}

// decoder, one set per launch (anchors first): the CTX_WPB_DEC streams from `first` on, below `end`, of set SET of the image, in
// the set's own numbering (the full decoders: a group of the set, first = grp * CTX_WPB_DEC, end = nst[SET]; the window decoder: a
// group of its selection — no wave decodes or writes a stream outside [first, end)).  One group per table load at every stream
// length.  A stream of S <= 2048 symbols (at most 4352 bytes) fits the 8 KB ring whole: one fill, and the refill
// test of the block loop never fires.
// LDS: 8 + 64 KB of tables + 8 rings of 8 KB = 136 KB of the CU's 160: one workgroup of 8 waves per CU, at every S.  The symbol of a slot
// comes from ONE table read (16 classes x 4096 slots = 64 KB of LDS, shared by the workgroup's eight waves; round 3 read the first
// symbol of a 16-slot bucket and walked the cumulative table from there — up to a dozen dependent LDS round trips per step on a
// flat class, with six waves per CU to hide them behind).  SET is a template parameter so that the geometry's per-set fields are
// picked at compile time: indexed by a kernel argument, the row went to scratch memory (profiles/ragged_ctx_resource_usage.txt).
constexpr uint32_t CTX_WPB_DEC = 8;
template <int SET>
__device__ __forceinline__ void ctx_decode_body(const CtxImage &im, uint32_t first, uint32_t end)
{
    constexpr int set = SET;
    const CtxGeom &g = im.g;
    const uint8_t *payload = im.slot + SICN_CODEC_HEADER_BYTES + CTX_TABLE_BYTES + 4 * (size_t)(g.nst[0] + g.nst[1]);
    const uint8_t *scale = im.scale, *tst = im.w.tst;
    const uint32_t *offsets = im.w.offsets, *tfc = im.w.tfc;
    uint8_t *lat = im.lat;
    uint32_t *meta = im.w.meta;
    __shared__ uint32_t fc[NCLS * 128];
    __shared__ __attribute__((aligned(16))) uint8_t stb[NCLS * 4096];
    __shared__ __attribute__((aligned(16))) uint16_t words_all[CTX_WPB_DEC][RING_WORDS];   // one ring per wave, see ransw_decode_body
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, sidx = first + wv, st = sidx + (set ? g.nst[0] : 0);
    {
        const uint4 *b = reinterpret_cast<const uint4 *>(tst);   // the workspace block is 16-byte aligned (ctx_carve)
        for (uint32_t i = threadIdx.x; i < NCLS * 128; i += 64 * CTX_WPB_DEC) fc[i] = tfc[i];
        for (uint32_t i = threadIdx.x; i < NCLS * 256; i += 64 * CTX_WPB_DEC) reinterpret_cast<uint4 *>(stb)[i] = b[i];
    }
    __syncthreads();
    if (sidx >= end) return;   // (no block barrier below this line)
    uint16_t *words = words_all[wv];
    const uint32_t begin = sidx * g.S, cnt = min(g.S, g.nsym[set] - begin), blocks = (cnt + 255) / 256;
    const uint32_t off = offsets[st], len = offsets[st + 1] - off, payload_bytes = meta[1];
    if (len < 256 || (len & 1) || (off & 1) || len > wstream_cap(g.S) || (unsigned long long)off + len > payload_bytes) {
        if (lane == 0) atomicOr(&meta[3], 1u);
        return;
    }
    const uint32_t nwords = len / 2;
    const uint16_t *src = (const uint16_t *)(payload + off);
    uint32_t loaded = ring_fill(words, src, 0, min(nwords, RING_WORDS), lane);
    wave_lds_sync();
    uint32_t x = words[2 * lane] | ((uint32_t)words[2 * lane + 1] << 16), wpos = 128;
    const unsigned long long below = (1ull << lane) - 1;
    bool bad = false;
    // the classes of a block come from global memory (the scale map and, for the non-anchors, the four anchor neighbours the
    // previous launch decoded): requested ONE BLOCK AHEAD.  Round 3 fetched them at the top of the block they were needed in —
    // with ~6 streams per CU in flight (a set of a 4K latent has 190 streams) that latency, 64 times per stream, was half of
    // the kernel.
    auto locate = [&](uint32_t q, uint32_t &o, uint32_t &cls4) -> bool {
        const uint32_t j = q * 256 + lane * 4;
        o = cls4 = 0;
        if (j >= cnt) return false;      // cnt is a multiple of 4
        const uint32_t e = begin + j, px = e / g.C, ch = e - px * g.C;
        uint32_t y, xx;
        ctx_pixel(set, px, g.W, y, xx);
        o = (y * g.W + xx) * g.C + ch;
        cls4 = ctx_class4(set, lat, scale, g.W, g.H, g.C, y, xx, o);
        return true;
    };
    uint32_t o_next = 0, cls_next = 0;
    bool mine_next = blocks ? locate(0, o_next, cls_next) : false;
    for (uint32_t q = 0; q < blocks; q++) {
        if (loaded < nwords && loaded - min(wpos, loaded) < 4 * 64) {
            wave_lds_sync();
            loaded = ring_fill(words, src, loaded, min(nwords, wpos + RING_WORDS), lane);
            wave_lds_sync();
        }
        const bool mine = mine_next;
        const uint32_t cls4 = cls_next, o = o_next;
        mine_next = q + 1 < blocks ? locate(q + 1, o_next, cls_next) : false;
        uint32_t out4 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (mine) {
                const uint32_t base = ((cls4 >> (8 * k)) & 15u) * 128, v = x & 4095u;
                const uint32_t sy = stb[(base << 5) + v] & 127u;   // (a slot no symbol covers holds anything: caught by the range test)
                const uint32_t t = fc[base + sy], f = t & 0xFFFFu;
                bad |= f == 0 || v < (t >> 16) || v >= (t >> 16) + f;   // a class without a table, or a hole in it
                out4 |= sy << (8 * k);
                x = f * (x >> PROB_BITS) + v - (t >> 16);
            }
            const bool need = mine && x < RANSW_L;
            const unsigned long long mask = __ballot(need);
            if (need) {
                const uint32_t idx = wpos + (uint32_t)__popcll(mask & below);
                if (idx < loaded)
                    x = (x << 16) | words[idx & (RING_WORDS - 1)];
                else
                    bad = true;
            }
            wpos += (uint32_t)__popcll(mask);
        }
        if (mine) *reinterpret_cast<uint32_t *>(lat + o) = out4;
    }
    if (bad || x != RANSW_L || wpos != nwords) atomicOr(&meta[3], 1u);
}

// ---- the bookkeeping stages: the steps of k_codec_body.hpp on one CtxImage.  `status`: the batch's sicn_codec_status array --------
// encoder, first on the stream, 256 lanes: the statistics block and the class histograms behind it (contiguous), which the next stage adds to
__device__ __forceinline__ void ctx_clear_body(const CtxImage &im)
{
    for (uint32_t i = threadIdx.x; i < STATS_WORDS + 16 + NCLS * 128; i += 256) im.w.hist[i] = 0;
}

// One workgroup of 1024.  Encoder: stream lengths -> offsets, the container's length table and payload-bytes field, status[img].bytes.
// Decoder: the container's length table -> offsets (entries above a stream's cap are an error; a slot the parse stage found too short is not read).
__device__ __forceinline__ void ctx_scan_body(const CtxImage &im, uint32_t *status, uint32_t img, bool dec)
{
    const CtxWorkspace &w = im.w;
    const uint32_t ns = im.g.nst[0] + im.g.nst[1];
    uint8_t *table = im.slot + SICN_CODEC_HEADER_BYTES + CTX_TABLE_BYTES;
    if (dec)
        scan_body(nullptr, table, ns, w.offsets, nullptr, nullptr, wstream_cap(im.g.S), w.meta + 3, nullptr, 0u, (w.meta[0] & 0x100u) != 0);
    else
        scan_body(w.lens, nullptr, ns, w.offsets, table, im.slot + 40, 0xFFFFFFFFu, nullptr, status + 2 * (size_t)img + 1,
                  (uint32_t)(SICN_CODEC_HEADER_BYTES + CTX_TABLE_BYTES) + 4 * ns, false);
}

// stream `st` of the image, anchors and non-anchors numbered through, by one workgroup of 256
__device__ __forceinline__ void ctx_compact_body(const CtxImage &im, uint32_t st)
{
    const uint32_t ns = im.g.nst[0] + im.g.nst[1];
    compact_body(im.w.scratch, im.w.lens, im.w.offsets, im.slot + SICN_CODEC_HEADER_BYTES + CTX_TABLE_BYTES + 4 * (size_t)ns, wstream_cap(im.g.S), st);
}

// decoder back end, ONE lane: the verdict of the whole image -> status[img] = {error, n_symbols}
__device__ __forceinline__ void ctx_finish_body(const CtxImage &im, uint32_t *status, uint32_t img)
{
    dec_finish_body(im.w.meta, im.w.sums, im.w.offsets, status + 2 * (size_t)img, im.g.W * im.g.H * im.g.C, im.g.nst[0] + im.g.nst[1]);
}
// the same for a window of the image's streams holding `symbols`: the container's fixed part and the selected streams; bit 7 is never set
__device__ __forceinline__ void ctx_finish_window_body(const CtxImage &im, uint32_t *status, uint32_t img, uint32_t symbols)
{
    uint32_t err = im.w.meta[0];
    if (im.w.meta[3]) err |= 32;                                              // a selected stream, or an entry of the length table
    if (im.w.offsets[im.g.nst[0] + im.g.nst[1]] != im.w.meta[1]) err |= 64;   // the length table does not add up to the payload
    status[2 * (size_t)img] = err;
    status[2 * (size_t)img + 1] = symbols;
}

}  // namespace
