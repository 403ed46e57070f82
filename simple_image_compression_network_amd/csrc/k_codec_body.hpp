// The rANS-W coder's device code, shared by the uniform batch kernels (sicn_codec.hip: blockIdx.y = image, every image of one shape,
// pointers advancing by uniform strides) and the ragged ones (k_ragged_codec.hip: a flat grid over the work items of n images of n
// shapes, each image found through a table).  Every stage is a __device__ function of a small per-image context (EncImage /
// DecImage: the image's latent, sizes, workspace block, container slot and status entry, already resolved to pointers) and of the
// stream or statistics-row index INSIDE the image.  Both kinds of kernel name an image by one CoderRow and turn it into that context
// with enc_image() / dec_image(); they differ only in where the row comes from (UniformBatch: computed; ragged: loaded).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sicn.h"
#include "../../include/sicn_codec.h"
#include "k_ragged_common.hpp"

namespace {

constexpr uint32_t SS = SICN_CODEC_STREAM_SYMBOLS;
constexpr uint32_t CAP = 2 * SS + 16;  // scratch bytes per stream (12-bit worst case is 1.5 B/symbol + 4)
constexpr uint32_t WSS = SICN_CODEC_WSTREAM_SYMBOLS;   // mode 3: 64 lanes x 256 steps
constexpr uint32_t WCAP = 2 * WSS + 256;               // at most one 16-bit word per symbol + the 64 final states
constexpr uint32_t RANSW_L = 1u << 16;
inline uint32_t stream_symbols(int mode) { return mode == SICN_CODEC_RANSW ? WSS : SS; }
// mode 3 with the encoder's choice of stream length (header dword 9): a power of two, 1024 .. 16384 symbols.  Shorter streams =
// more waves = a shorter serial chain for a small latent, + 260 bytes per stream (64 final states, one length entry).
__host__ __device__ inline bool wstream_ok(uint32_t wss) { return wss >= 1024u && wss <= WSS && (wss & (wss - 1u)) == 0; }
__host__ __device__ inline uint32_t wstream_cap(uint32_t wss) { return 2u * wss + 256u; }   // scratch bytes per stream (= WCAP at 16384)
constexpr uint32_t RANS_L = 1u << 23;
constexpr int PROB_BITS = 12;
constexpr uint32_t ADLER_MOD = 65521u;
// rANS modes: ceil(n / stream symbols) * scratch capacity must stay below 2^32 (32-bit stream offsets):
// 0x7F000000 / 16384 * 33024 = 0x7F000000 / 1024 * 2064 = 4 294 705 152 < 2^32
constexpr uint32_t MAX_RANS_SYMBOLS = 0x7F000000u;
static_assert((unsigned long long)(MAX_RANS_SYMBOLS / WSS) * WCAP < (1ull << 32), "mode 3 offsets would wrap");
static_assert((unsigned long long)(MAX_RANS_SYMBOLS / SS) * CAP < (1ull << 32), "mode 2 offsets would wrap");
// Asynchronous paths, small stream counts: a small image's coder time is launch latency (ten kernels of which seven were 5 us
// bookkeeping stages), so up to this many streams per image the scans are done by the consumers themselves (every wave sums the
// length table up to its own stream) and the statistics are per-workgroup rows instead of atomics on a block that has to be
// cleared first: encode 6 -> 4 launches, decode 4 -> 2.
constexpr uint32_t SELF_SCAN_MAX = 2048;
constexpr uint32_t STAT_ROWS = 64;                 // at most this many statistics workgroups (rows) per image in row mode
constexpr uint32_t STAT_ROW_WORDS = 256 + 4;       // hist[256], then s1, s2 as two u64
inline uint32_t stat_rows(uint32_t n) { const uint32_t r = n / 16384u; return r < 1 ? 1 : r > STAT_ROWS ? STAT_ROWS : r; }   // rows of an n-symbol image

struct Workspace {  // device pointers carved out of the caller's workspace
    uint32_t *hist;                // [256]
    unsigned long long *sums;      // [2]: sum d_i, sum (n-i) d_i, both reduced mod 65521 per lane
    uint16_t *freq;                // [128]
    uint32_t *meta;                // [16] async paths: [0] error flags, [1] sanitised payload bytes, [2] header adler32
    uint32_t *lens;                // [ns]
    uint32_t *offsets;             // [ns + 1]
    uint8_t *scratch;              // [ns][CAP]
    uint32_t *rows;                // [STAT_ROWS][STAT_ROW_WORDS] async encode, row mode: per-workgroup histograms and checksum sums
};

__host__ __device__ inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

__host__ __device__ inline size_t carve(Workspace &w, void *base, uint32_t ns, size_t scratch_per_stream)
{
    uint8_t *p = (uint8_t *)base;
    size_t off = 0;
    w.hist = (uint32_t *)(p + off); off += 1024;
    w.sums = (unsigned long long *)(p + off); off += 64;
    w.freq = (uint16_t *)(p + off); off += 256;
    w.meta = (uint32_t *)(p + off); off += 64;
    w.lens = (uint32_t *)(p + off); off += align_up(4 * (size_t)ns + 4, 64);
    w.offsets = (uint32_t *)(p + off); off += align_up(4 * (size_t)ns + 4, 64);
    w.scratch = p + off;
    off += align_up((size_t)ns * scratch_per_stream, 64);
    w.rows = (uint32_t *)(p + off);
    off += (size_t)STAT_ROWS * STAT_ROW_WORDS * 4;
    return off;
}

// ---- one image as the stages see it ---------------------------------------------------------------------------------------
struct EncImage {
    const uint8_t *lat;            // [n] symbols
    uint32_t n, ns, wss;
    uint8_t *scratch;              // workspace block: [ns][wstream_cap(wss)]
    uint32_t *lens;                //                  [ns]
    const uint32_t *rows;          //                  [n_rows][STAT_ROW_WORDS], or nullptr: the table comes from `freq`
    const uint16_t *freq;          //                  [128] (only without rows)
    uint32_t n_rows;
    uint8_t *out;                  // container slot
    uint32_t *status;              // sicn_codec_status {error, bytes} of this image
    uint32_t lat_w, lat_h, lat_c, img_w, img_h;
};
struct DecImage {
    const uint8_t *c;              // container slot: header, at + 40 its payload-bytes field `pbf`, at + 48 the frequency table
    const uint8_t *pbf, *freq_bytes, *payload;   // `freq_bytes`, behind it the length table [ns], behind that the `payload`
    uint32_t slot_cap;             // bytes of the slot: nothing is read beyond min(*valid, slot_cap)
    const uint32_t *valid;         // valid bytes of this slot (e.g. the encoder's status.bytes), or nullptr = slot_cap
    uint8_t *lat;                  // [n] symbols out
    uint32_t n, ns, wss, lat_w, lat_h, lat_c;
    uint32_t *err;                 // self form: [ns] per-stream verdicts; else one word of error flags (atomics)
    unsigned long long *sums;      // self form: [2 ns] per-stream checksum sums; else [2] (atomics)
    const uint32_t *offsets;       // [ns + 1] from ransw_scan_body (not in the self form)
    const uint32_t *meta;          // dec_parse_body's verdict (not in the self form)
    uint32_t *status;              // sicn_codec_status {error, bytes} of this image
};

// ---- one image as the kernels name it -------------------------------------------------------------------------------------
// Sizes and 64-bit byte offsets into the latent tensor, the slot buffer and the workspace; the workspace block of an image is what
// carve() gives for (ns, wstream_cap(wss)).  The ragged coder keeps a table of these (k_ragged_codec.hip).
struct CoderRow {
    uint64_t lat_off, slot_off, ws_off;
    uint32_t n, ns, wss, slot_cap;
    uint32_t lat_w, lat_h, lat_c, img_w, img_h;
    uint32_t first_stream, first_row, n_rows;   // ragged: the image's first work items in the flat grids; n_rows: its statistics rows
};
// a row of a table in memory (the ragged kernels), every field wave-uniform
__device__ __forceinline__ CoderRow load_row(const CoderRow *__restrict__ rows, uint32_t img)
{
    const CoderRow *r = rows + img;
    return CoderRow{uni(r->lat_off), uni(r->slot_off), uni(r->ws_off), uni(r->n), uni(r->ns), uni(r->wss), uni(r->slot_cap),
                    uni(r->lat_w), uni(r->lat_h), uni(r->lat_c), uni(r->img_w), uni(r->img_h), uni(r->first_stream),
                    uni(r->first_row), uni(r->n_rows)};
}
// A uniform batch (sicn_codec.hip: blockIdx.y = image, every image of one shape) is image 0's row and three byte strides.  Passed by
// value, so it lives in kernel-argument SGPRs.  `scan`: the form above SELF_SCAN_MAX streams (no statistics rows; a scan kernel in front).
struct UniformBatch {
    CoderRow row0;
    uint64_t s_lat, s_slot, s_ws;
    uint32_t scan;
};
__device__ __forceinline__ CoderRow batch_row(const UniformBatch &b)
{
    CoderRow r = b.row0;
    r.lat_off += blockIdx.y * b.s_lat; r.slot_off += blockIdx.y * b.s_slot; r.ws_off += blockIdx.y * b.s_ws;
    return r;
}

// scan: the table comes from enc_header_body's `freq`, not from statistics rows
__device__ __forceinline__ EncImage enc_image(const CoderRow &r, const uint8_t *latents, uint8_t *containers, uint32_t *status,
                                              uint8_t *workspace, uint32_t img, bool scan = false)
{
    Workspace w;
    carve(w, workspace + r.ws_off, r.ns, wstream_cap(r.wss));
    EncImage im;
    im.lat = latents + r.lat_off;
    im.n = r.n; im.ns = r.ns; im.wss = r.wss;
    im.scratch = w.scratch;
    im.lens = w.lens;
    im.rows = scan ? nullptr : w.rows;
    im.freq = scan ? w.freq : nullptr;
    im.n_rows = r.n_rows;
    im.out = containers + r.slot_off;
    im.status = status + 2 * (size_t)img;
    im.lat_w = r.lat_w; im.lat_h = r.lat_h; im.lat_c = r.lat_c; im.img_w = r.img_w; im.img_h = r.img_h;
    return im;
}

// valid: a sicn_codec_status array whose .bytes bound the slots, or nullptr.  scan: dec_parse_body and ransw_scan_body ran in front, the
// streams report through the statistics block (meta[3], sums) instead of per-stream words
__device__ __forceinline__ DecImage dec_image(const CoderRow &r, const uint8_t *containers, const uint32_t *valid, uint8_t *latents,
                                              uint32_t *status, uint8_t *workspace, uint32_t img, bool scan = false)
{
    Workspace w;
    carve(w, workspace + r.ws_off, r.ns, wstream_cap(r.wss));
    DecImage im;
    im.c = containers + r.slot_off;
    im.pbf = im.c + 40;
    im.freq_bytes = im.c + SICN_CODEC_HEADER_BYTES;
    im.payload = im.freq_bytes + 256 + 4 * (size_t)r.ns;
    im.slot_cap = r.slot_cap;
    im.valid = valid ? valid + 2 * (size_t)img + 1 : nullptr;   // sicn_codec_status.bytes
    im.lat = latents + r.lat_off;
    im.n = r.n; im.ns = r.ns; im.wss = r.wss;
    im.lat_w = r.lat_w; im.lat_h = r.lat_h; im.lat_c = r.lat_c;
    im.err = scan ? w.meta + 3 : w.lens;                                   // self: [ns] per-stream verdicts
    im.sums = scan ? w.sums : (unsigned long long *)w.scratch;            // self: [2 ns]; the scratch slots (>= 2304 B each) are idle in a decode
    im.offsets = scan ? w.offsets : nullptr;
    im.meta = scan ? w.meta : nullptr;
    im.status = status + 2 * (size_t)img;
    return im;
}

// ---- stages ---------------------------------------------------------------------------------------------------------------
// histogram (256 bins) + the two sums adler32 is made of; grid-stride over 16-byte groups (consecutive lanes read
// consecutive groups); zeros — half of a ReLU latent — are counted in a register instead of hammering one LDS bin.
// Workgroup `bx` of the `nb` that share one image.  row != nullptr (row mode): this workgroup's own statistics row.
__device__ __forceinline__ void stats_body(const uint8_t *__restrict__ lat, uint32_t n, uint32_t *__restrict__ hist,
                                           unsigned long long *__restrict__ sums, uint32_t *__restrict__ row, uint32_t bx, uint32_t nb)
{
    // 8 copies of the histogram, copy = lane & 7, at a pitch of 257 words: latents are skewed (a few small values carry most
    // of the mass), so lanes of one wave mostly hit the SAME bin — with one copy those LDS atomics serialise; copies of a bin
    // sit in 8 different banks
    __shared__ uint32_t h[8 * 257];
    for (int i = threadIdx.x; i < 8 * 257; i += 256) h[i] = 0;
    uint32_t *hl = h + (threadIdx.x & 7) * 257;
    __syncthreads();
    unsigned long long s1 = 0, s2 = 0;
    uint32_t zeros = 0;
    const bool vec = (reinterpret_cast<uintptr_t>(lat) & 15) == 0;
    const uint32_t groups = vec ? n / 16 : 0;
    for (uint32_t g = bx * 256 + threadIdx.x; g < groups; g += nb * 256) {
        const uint4 q = reinterpret_cast<const uint4 *>(lat)[g];
        const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t d = (w4[k >> 2] >> (8 * (k & 3))) & 255u;
            if (d) {
                atomicAdd(&hl[d], 1u);
                s1 += d;
                s2 += (unsigned long long)(n - (16 * g + k)) * d;   // < 2^39 per term, far fewer than 2^25 terms per lane
            } else
                zeros++;
        }
    }
    for (uint32_t i = 16 * groups + bx * 256 + threadIdx.x; i < n; i += nb * 256) {
        const uint32_t d = lat[i];
        if (d) {
            atomicAdd(&hl[d], 1u);
            s1 += d;
            s2 += (unsigned long long)(n - i) * d;
        } else
            zeros++;
    }
    s2 %= ADLER_MOD;
    // one atomic per wave, not per lane: wavefront-level reduction first
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        s1 += __shfl_down(s1, d);
        s2 += __shfl_down(s2, d);
        zeros += __shfl_down(zeros, d);
    }
    if ((threadIdx.x & 63) == 0 && zeros) atomicAdd(&h[0], zeros);
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) total += h[c * 257 + threadIdx.x];
    if (row) {   // row mode: this workgroup's own row, plain stores (nothing to clear, no atomics on shared words)
        __shared__ unsigned long long ws1[4], ws2[4];
        if ((threadIdx.x & 63) == 0) { ws1[threadIdx.x >> 6] = s1; ws2[threadIdx.x >> 6] = s2 % ADLER_MOD; }
        __syncthreads();
        row[threadIdx.x] = total;
        if (threadIdx.x == 0) {
            unsigned long long *q = (unsigned long long *)(row + 256);
            q[0] = ws1[0] + ws1[1] + ws1[2] + ws1[3];
            q[1] = (ws2[0] + ws2[1] + ws2[2] + ws2[3]) % ADLER_MOD;
        }
        return;
    }
    if ((threadIdx.x & 63) == 0) {
        if (s1) atomicAdd(&sums[0], s1);
        if (s2) atomicAdd(&sums[1], s2 % ADLER_MOD);
    }
    if (total) atomicAdd(&hist[threadIdx.x], total);
}

// ---- rANS-W: one wave (= one 64-lane workgroup) per stream -----------------------------------------
// Lane l codes symbols 256 q + 4 l + k (k = 0..3) in steps 4 q + k: one aligned dword of symbols per lane and
// 256-symbol block.  The 16-bit words live in LDS while the stream is coded (their positions are data
// dependent: rank of the lane among the renormalising lanes = popcount of a ballot) and move between LDS and
// global memory in whole coalesced runs.
struct RanswTab {
    uint32_t fc[128];   // freq | cum << 16
    uint32_t rcp[128];  // m = min(2^32 - 1, floor(2^32 / freq)): umulhi(x, m) is floor(x / freq) or one less, never more (see ransw_div)
};

// Exact x / f for x < 2^32, 1 <= f <= 4096, without an integer divide.  m = floor(2^32 / f) (2^32 - 1 for f = 1)
// satisfies m <= 2^32 / f, so e = floor(x m / 2^32) <= floor(x / f): the estimate is NEVER too large; and
// x / f - x m / 2^32 = x (2^32 / f - m) / 2^32 < x / 2^32 < 1, so e >= floor(x / f) - 1: ONE fix-up step is enough.
// (Round 1 used a float reciprocal whose rounded product could exceed the quotient for 295 of the 4096
// frequencies, e.g. f = 3815, x = 250046544; tests/test_codec.py::test_ransw_div_exhaustive covers all f.)
__host__ __device__ __forceinline__ uint32_t ransw_rcp(uint32_t f)
{
    return f <= 1 ? (f ? 0xFFFFFFFFu : 0u) : (uint32_t)(0x100000000ull / f);
}

__host__ __device__ __forceinline__ uint32_t ransw_div(uint32_t x, uint32_t f, uint32_t m, uint32_t &r)
{
    uint32_t q = (uint32_t)(((unsigned long long)x * m) >> 32);   // v_mul_hi_u32
    r = x - q * f;
    if (r >= f) { q++; r -= f; }
    return q;
}

__device__ __forceinline__ void ransw_build(RanswTab &t, const uint16_t *freq, int lane)
{
    // exclusive prefix sum of 128 frequencies by one wave: two elements per lane + wavefront scan
    const uint32_t f0 = freq[2 * lane], f1 = freq[2 * lane + 1];
    uint32_t incl = f0 + f1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    const uint32_t c0 = incl - f0 - f1;
    t.fc[2 * lane] = f0 | (c0 << 16);
    t.fc[2 * lane + 1] = f1 | ((c0 + f0) << 16);
    t.rcp[2 * lane] = ransw_rcp(f0);
    t.rcp[2 * lane + 1] = ransw_rcp(f1);
}

// The 16-bit words of a stream pass through a small LDS RING (8 KB) instead of a buffer sized for the worst case (33 KB):
// the worst case still fits the stream's scratch slot in global memory, but a wave now costs 9 KB (mode 3) / 24 KB (mode 4) of
// LDS, so a CU holds all of its streams at once (a 4K latent gives a CU about 12) instead of 4 at a time — the coders are
// latency-bound serial chains, occupancy is their only source of throughput.
//   encoder: words are produced at DEcreasing global word indices gpos-1, gpos-2, ..; ring slot = index % RING_WORDS; whenever
//            fewer than one step's worth (64) of slots is left, the words [gpos, top) go out to the scratch slot.
//   decoder: words are consumed at INcreasing indices; before every block of 4 steps (<= 256 words) the ring is topped up.
constexpr uint32_t RING_WORDS = 4096;
__device__ __forceinline__ void ring_flush(const uint16_t *ring, uint16_t *dst, uint32_t gpos, uint32_t top, uint32_t lane)
{
    // word i of the stream sits at ring[i % RING_WORDS] and goes to dst[i]: 8-word groups at multiples of 8 are contiguous and
    // 16-byte aligned on both sides (RING_WORDS % 8 == 0, dst is a scratch slot at a 16-byte multiple), so the body moves 16 bytes
    // per lane and instruction; the ragged head and tail go word by word (round 4: the whole run used to go 2 bytes at a time)
    const bool vec = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const uint32_t a = vec ? min(top, (gpos + 7u) & ~7u) : top, b = vec ? max(a, top & ~7u) : top;
    for (uint32_t i = gpos + lane; i < a; i += 64) dst[i] = ring[i & (RING_WORDS - 1)];
    for (uint32_t i = a + 8 * lane; i < b; i += 8 * 64)
        *reinterpret_cast<uint4 *>(dst + i) = *reinterpret_cast<const uint4 *>(ring + (i & (RING_WORDS - 1)));
    for (uint32_t i = b + lane; i < top; i += 64) dst[i] = ring[i & (RING_WORDS - 1)];
}
__device__ __forceinline__ uint32_t ring_fill(uint16_t *ring, const uint16_t *src, uint32_t loaded, uint32_t upto, uint32_t lane)
{
    // the payload side is only 2-byte aligned (streams start at even container offsets): dwords when the source happens to be
    // 4-byte aligned relative to the ring's even word indices, else word by word
    if ((reinterpret_cast<uintptr_t>(src) & 3) == 0) {
        const uint32_t a = min(upto, (loaded + 1u) & ~1u), b = max(a, upto & ~1u);
        if (lane == 0 && loaded < a) ring[loaded & (RING_WORDS - 1)] = src[loaded];
        for (uint32_t i = a + 2 * lane; i < b; i += 128)
            *reinterpret_cast<uint32_t *>(ring + (i & (RING_WORDS - 1))) = *reinterpret_cast<const uint32_t *>(src + i);
        if (lane == 0 && b < upto) ring[b & (RING_WORDS - 1)] = src[b];
        return upto;
    }
    for (uint32_t i = loaded + lane; i < upto; i += 64) ring[i & (RING_WORDS - 1)] = src[i];
    return upto;
}

// ---- the encoder's per-symbol table: one 16-byte entry (ONE ds_read_b128) instead of two dword tables, and the renormalisation
// ---- test as a precomputed threshold.  Round 4: the step loop used to make two dependent LDS round trips per symbol (frequency,
// ---- then reciprocal, each behind an s_waitcnt and a branch); now the four entries of a block are fetched while the PREVIOUS
// ---- block's chain runs and the step itself is branch-free.
struct RanswEnt {
    uint32_t fc;    // freq | cum << 16
    uint32_t rcp;   // ransw_rcp(freq)
    uint32_t thr;   // a lane renormalises iff x > thr: freq * 2^20 - 1 (freq = 4096: never, 2^32 - 1; freq = 0: unused symbol)
    uint32_t pad;
};
__device__ __forceinline__ RanswEnt ransw_ent(uint32_t f, uint32_t c)
{
    return RanswEnt{f | (c << 16), ransw_rcp(f), (f == 0 || f >= 4096u) ? 0xFFFFFFFFu : (f << 20) - 1u, 0u};
}
// table of one wave from this lane's two frequencies (symbols 2 lane, 2 lane + 1): exclusive prefix sum by a wavefront scan
__device__ __forceinline__ void ransw_build_ent(RanswEnt *ent, uint32_t f0, uint32_t f1, int lane)
{
    uint32_t incl = f0 + f1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    const uint32_t c0 = incl - f0 - f1;
    ent[2 * lane] = ransw_ent(f0, c0);
    ent[2 * lane + 1] = ransw_ent(f1, c0 + f0);
}

// Histogram -> 12-bit frequencies exactly as `normalize` / sicl_or_normalize do it (same floor, same "largest first, lowest index
// on ties" correction walk), by ONE wave: lane l owns symbols 2l, 2l+1 (hh = their counts).  Returns the error bits (2 = no valid table).
__device__ __forceinline__ uint32_t normalize_wave(const uint32_t (&hh)[2], uint32_t n, uint32_t (&f)[2], int lane)
{
    uint32_t err = 0;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint32_t h = hh[k];
        unsigned long long v = (h && n) ? ((unsigned long long)h * 4096u) / n : 0;
        if (h && v == 0) v = 1;
        f[k] = (uint32_t)v;
    }
    int sum = (int)(f[0] + f[1]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    int diff = n ? 4096 - sum : 0;
    for (int it = 0; it < 200 && diff != 0; it++) {
        // candidate of this lane: f > 0 and (diff > 0 or f > 1); key = (f << 8) | (255 - index): max key = largest f, lowest index
        uint32_t key = 0;
#pragma unroll
        for (int k = 0; k < 2; k++)
            if (f[k] > 0 && (diff > 0 || f[k] > 1)) key = max(key, (f[k] << 8) | (uint32_t)(255 - (2 * lane + k)));
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, d));
        if (key == 0) { err |= 2; break; }
        const int best = 255 - (int)(key & 255u), fb = (int)(key >> 8);
        const int step = diff > 0 ? diff : (diff < 1 - fb ? 1 - fb : diff);
        if ((best >> 1) == lane) f[best & 1] = (uint32_t)(fb + step);
        diff -= step;
    }
    if (diff != 0) err |= 2;
    return err;
}

// container header (dwords 0..11 but 10 = payload bytes, written by the scan / compaction stage) + frequency table, by one wave
__device__ __forceinline__ void write_header_wave(uint8_t *out, const uint32_t (&f)[2], unsigned long long s1, unsigned long long s2,
                                                  uint32_t n, uint32_t ns, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t img_w,
                                                  uint32_t img_h, uint32_t wss, int lane)
{
    uint8_t *ft = out + SICN_CODEC_HEADER_BYTES + 4 * lane;
    ft[0] = (uint8_t)f[0]; ft[1] = (uint8_t)(f[0] >> 8); ft[2] = (uint8_t)f[1]; ft[3] = (uint8_t)(f[1] >> 8);
    if (lane < 12) {
        const uint32_t a = (uint32_t)((1 + s1) % ADLER_MOD), b = (uint32_t)((n % ADLER_MOD + s2) % ADLER_MOD);
        const uint32_t words[12] = {0x4C434953u /* "SICL" */, 1u | ((uint32_t)SICN_CODEC_RANSW << 16), img_w, img_h, lat_w, lat_h,
                                    lat_c, n, ns, wss, 0u, (b << 16) | a};
        if (lane != 10) {
            const uint32_t v = words[lane];
            uint8_t *p = out + 4 * lane;
            p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
        }
    }
}

// One stream (`st`) of one image by one wave.  With im.rows (the asynchronous encoder's row mode) every wave makes the frequency table
// from the statistics rows ITSELF (one launch less — the header kernel was 8.5 us of a 1080p encode, nearly all of it launch
// latency): it sums the rows and runs the (deterministic) normalisation; stream 0's wave also writes header, table and status.
__device__ __forceinline__ void ransw_encode_body(const EncImage &im, uint32_t st)
{
    const uint8_t *__restrict__ lat = im.lat;
    uint8_t *__restrict__ scratch = im.scratch;
    uint32_t *__restrict__ lens = im.lens;
    const uint32_t n = im.n, ns = im.ns, wss = im.wss;
    __shared__ __attribute__((aligned(16))) RanswEnt ent[128];
    __shared__ __attribute__((aligned(16))) uint16_t words[RING_WORDS];
    const uint32_t lane = threadIdx.x;
    if (im.rows) {
        const uint32_t *rows = im.rows;
        uint32_t hh[2] = {0, 0}, hi = 0;
#pragma unroll 8
        for (uint32_t r = 0; r < im.n_rows; r++) {
            const uint32_t *row = rows + (size_t)r * STAT_ROW_WORDS;
            const uint2 two = *reinterpret_cast<const uint2 *>(row + 2 * lane);
            hh[0] += two.x;
            hh[1] += two.y;
            hi |= row[128 + lane] | row[192 + lane];
        }
        uint32_t f[2];
        uint32_t err = normalize_wave(hh, n, f, (int)lane) | (hi ? 1u : 0u);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) err |= (uint32_t)__shfl_xor((int)err, d);
        if (err) f[0] = f[1] = 0;   // zero-frequency symbols are skipped below: the kernel stays memory-safe
        ransw_build_ent(ent, f[0], f[1], (int)lane);
        if (st == 0) {              // header, table and encoder status of this image: once
            unsigned long long s1 = 0, s2 = 0;
            for (uint32_t r = lane; r < im.n_rows; r += 64) {
                const unsigned long long *q = (const unsigned long long *)(rows + (size_t)r * STAT_ROW_WORDS + 256);
                s1 += q[0];
                s2 += q[1];
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                s1 += __shfl_xor(s1, d);
                s2 += __shfl_xor(s2, d);
            }
            write_header_wave(im.out, f, s1, s2, n, ns, im.lat_w, im.lat_h, im.lat_c, im.img_w, im.img_h, wss, (int)lane);
            if (lane == 0) im.status[0] = err;
        }
    } else {
        const uint16_t *freq_g = im.freq;
        ransw_build_ent(ent, freq_g[2 * lane], freq_g[2 * lane + 1], (int)lane);
    }
    __syncthreads();
    const uint32_t wcap = wstream_cap(wss);
    const uint32_t begin = st * wss, cnt = min(wss, n - begin), blocks = (cnt + 255) / 256;
    const bool aligned = (reinterpret_cast<uintptr_t>(lat) & 3) == 0;   // begin is a multiple of the stream length (>= 1024)
    uint16_t *dst = (uint16_t *)(scratch + (size_t)st * wcap);
    uint32_t pos = wcap / 2, top = wcap / 2;   // word indices inside the scratch slot, the same in every lane: [pos, top) is in the ring
    uint32_t x = RANSW_L;
    const unsigned long long below = (1ull << lane) - 1;
    auto load4 = [&](uint32_t q) -> uint32_t {   // the lane's 4 symbols of block q (missing ones read as 0)
        const uint32_t j = q * 256 + lane * 4;
        if (aligned && j + 4 <= cnt) return *reinterpret_cast<const uint32_t *>(lat + begin + j);
        uint32_t v = 0;
        for (int k = 0; k < 4; k++)
            if (j + k < cnt) v |= (uint32_t)lat[begin + j + k] << (8 * k);
        return v;
    };
    const uint4 *ent4 = reinterpret_cast<const uint4 *>(ent);
    // software pipeline, two blocks deep: symbols of block q - 2 in flight from memory, table entries of block q - 1 in flight from
    // LDS, block q's chain on registers (symbols >= 128 are an error the statistics stage flags; they are masked here)
    uint32_t s_next = blocks > 1 ? load4(blocks - 2) : 0;
    uint4 e_cur[4];
    {
        const uint32_t s_cur = blocks ? load4(blocks - 1) : 0;
#pragma unroll
        for (int k = 0; k < 4; k++) e_cur[k] = ent4[(s_cur >> (8 * k)) & 127u];
    }
    for (uint32_t q = blocks; q-- > 0;) {
        const uint32_t s_next2 = q >= 2 ? load4(q - 2) : 0;
        uint4 e_next[4];
#pragma unroll
        for (int k = 0; k < 4; k++) e_next[k] = ent4[(s_next >> (8 * k)) & 127u];
        const int have = (int)min(4u, cnt - min(cnt, q * 256 + lane * 4));   // symbols of this lane in this block (4 but in a short last one)
#pragma unroll
        for (int k = 3; k >= 0; k--) {
            const uint32_t f = e_cur[k].x & 0xFFFFu, c = e_cur[k].x >> 16;
            const bool active = k < have && f != 0;          // f == 0 only for a latent the header stage rejected
            const bool emit = active && x > e_cur[k].z;      // x >= f * 2^20
            const unsigned long long mask = __ballot(emit);
            pos -= (uint32_t)__popcll(mask);
            if (emit) words[(pos + (uint32_t)__popcll(mask & below)) & (RING_WORDS - 1)] = (uint16_t)x;   // ascending lane order inside the step
            x = emit ? x >> 16 : x;
            uint32_t qq = __umulhi(x, e_cur[k].y);           // floor(x / f) or one less (ransw_div)
            uint32_t r = x - qq * f;
            const bool fix = r >= f;
            qq += fix ? 1u : 0u;
            r -= fix ? f : 0u;
            x = active ? (qq << PROB_BITS) + r + c : x;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) e_cur[k] = e_next[k];
        s_next = s_next2;
        if (top - pos > RING_WORDS - 4 * 64 - 128) {   // the next 4 steps (and the final states) must still fit
            __syncthreads();
            ring_flush(words, dst, pos, top, lane);
            __syncthreads();
            top = pos;
        }
    }
    pos -= 128;   // the 64 final states, lane 0 first (the word index may be odd: two halves)
    words[(pos + 2 * lane) & (RING_WORDS - 1)] = (uint16_t)x;
    words[(pos + 2 * lane + 1) & (RING_WORDS - 1)] = (uint16_t)(x >> 16);
    __syncthreads();
    ring_flush(words, dst, pos, top, lane);
    if (lane == 0) lens[st] = (wcap / 2 - pos) * 2;
}

// BIGTAB (the latency form, taken when an image's streams are few enough that occupancy does not matter): ONE 4096-entry dword
// table v -> symbol | freq << 7 | (v - cum) << 20 instead of the byte table v -> symbol followed by the symbol's (freq, cum): a
// decode step's chain is table -> multiply-add -> renormalisation word, and the second dependent LDS round trip is gone.  16 KB of
// LDS more per wave (5 waves per CU instead of 12), so large batches keep the two-table form, whose latency the other waves hide.
// One stream (`st`) of one image by one wave.
// self != 0 (the asynchronous path up to SELF_SCAN_MAX streams): NO parse and NO scan kernel ran before this one — the
// wave bounds the slot itself (valid bytes, header payload field), sums the length table up to its own stream, and reports
// through per-stream words (im.err[st], im.sums[2 st .. 2 st + 1], plain stores: nothing has to be cleared beforehand);
// dec_finish_self_body then validates header and table and folds the per-stream words into the status.
template <bool BIGTAB>
__device__ __forceinline__ void ransw_decode_body(const DecImage &im, uint32_t st, int self)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t n = im.n, ns = im.ns, wss = im.wss;
    const uint8_t *__restrict__ payload = im.payload, *__restrict__ freq_bytes = im.freq_bytes;
    // header field "payload bytes" of this image's container: no stream may reach beyond it (nor beyond the slot's valid bytes, which
    // bound the field below), whatever the untrusted length table says
    const uint8_t *__restrict__ pbf = im.pbf;
    uint32_t *__restrict__ err = im.err;
    if (self) {
        err += st;
        const size_t fixed = SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)ns;
        const uint32_t valid = im.valid ? min(*im.valid, im.slot_cap) : im.slot_cap;
        if (valid < fixed) {   // nothing of this slot may be read
            if (lane == 0) *err = 1u;
            return;
        }
    }
    uint32_t payload_bytes = pbf[0] | ((uint32_t)pbf[1] << 8) | ((uint32_t)pbf[2] << 16) | ((uint32_t)pbf[3] << 24);
    if (!self) payload_bytes = min(payload_bytes, im.meta[1]);   // scan form: clamped by the parse stage
    if (self) {
        const size_t fixed = SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)ns;
        const uint32_t valid = im.valid ? min(*im.valid, im.slot_cap) : im.slot_cap;
        if ((size_t)payload_bytes > (size_t)valid - fixed) payload_bytes = 0;   // what dec_parse_body's meta[1] says
    }
    const uint32_t *__restrict__ offsets = im.offsets;
    uint8_t *__restrict__ lat = im.lat;
    __shared__ RanswTab tab;
    __shared__ uint16_t freq[128];
    __shared__ __attribute__((aligned(16))) uint8_t slot[4096];
    __shared__ __attribute__((aligned(16))) uint16_t words[RING_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t big[BIGTAB ? 4096 : 4];
    freq[2 * lane] = (uint16_t)(freq_bytes[4 * lane] | (freq_bytes[4 * lane + 1] << 8));
    freq[2 * lane + 1] = (uint16_t)(freq_bytes[4 * lane + 2] | (freq_bytes[4 * lane + 3] << 8));
    __syncthreads();
    ransw_build(tab, freq, (int)lane);
    __syncthreads();
    for (int k = 0; k < 2; k++) {   // slot[c .. c + f) = symbol: 16 bytes per store in the middle (one symbol of a ReLU latent owns
        const uint32_t t = tab.fc[2 * lane + k], f = t & 0xFFFFu, c = t >> 16;   // half the table: 2048 byte stores by one lane
        const uint32_t e = min(c + f, 4096u), sy = (uint32_t)(2 * lane + k);     // were a third of a short stream's decode)
        uint32_t v = c;
        for (; v < e && (v & 15u); v++) slot[v] = (uint8_t)sy;
        const uint32_t pat = sy * 0x01010101u;
        for (; v + 16 <= e; v += 16) *reinterpret_cast<uint4 *>(slot + v) = make_uint4(pat, pat, pat, pat);
        for (; v < e; v++) slot[v] = (uint8_t)sy;
    }
    if constexpr (BIGTAB) {   // expand: entry v = symbol | freq << 7 | (v - cum) << 20 (7 + 13 + 12 bits), four consecutive v per lane and round
        __syncthreads();
#pragma unroll 4
        for (uint32_t v0 = 4 * lane; v0 < 4096; v0 += 256) {
            const uint32_t s4 = *reinterpret_cast<const uint32_t *>(slot + v0);
            uint4 o;
            uint32_t *ov = reinterpret_cast<uint32_t *>(&o);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t sy = (s4 >> (8 * k)) & 255u, t = tab.fc[sy & 127u];
                ov[k] = sy | ((t & 0xFFFFu) << 7) | ((v0 + k - (t >> 16)) << 20);
            }
            *reinterpret_cast<uint4 *>(big + v0) = o;
        }
    }
    const uint32_t begin = st * wss, cnt = min(wss, n - begin), blocks = (cnt + 255) / 256;
    uint32_t off, len;
    if (self) {   // exclusive prefix sum of the length table up to this stream, entries above the cap counting as 0 (as in scan_body)
        const uint8_t *table = freq_bytes + 256;
        const uint32_t cap = wstream_cap(wss);
        auto entry = [&](uint32_t i) {
            const uint8_t *q = table + 4 * (size_t)i;
            const uint32_t v = q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
            return v > cap ? 0u : v;
        };
        uint32_t sum = 0;
        if ((reinterpret_cast<uintptr_t>(table) & 3) == 0) {   // the usual case (slots at 4-byte multiples): one load per entry
            const uint32_t *t32 = reinterpret_cast<const uint32_t *>(table);
#pragma unroll 8
            for (uint32_t i = lane; i < st; i += 64) {
                const uint32_t v = t32[i];
                sum += v > cap ? 0u : v;
            }
        } else
            for (uint32_t i = lane; i < st; i += 64) sum += entry(i);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        off = sum;
        len = entry(st);
    } else {
        off = offsets[st];
        len = offsets[st + 1] - off;
    }
    if (len < 256 || (len & 1) || (off & 1) || len > wstream_cap(wss) ||
        (unsigned long long)off + len > payload_bytes) {   // streams start at even container offsets
        if (lane == 0) {
            if (self) *err = 1u; else atomicOr(err, 1u);
        }
        return;
    }
    const uint32_t nwords = len / 2;
    const uint16_t *src = (const uint16_t *)(payload + off);
    uint32_t loaded = ring_fill(words, src, 0, min(nwords, RING_WORDS), lane);
    __syncthreads();
    uint32_t x = words[2 * lane] | ((uint32_t)words[2 * lane + 1] << 16);
    uint32_t wpos = 128;
    const unsigned long long below = (1ull << lane) - 1;
    const bool aligned = (reinterpret_cast<uintptr_t>(lat) & 3) == 0;
    bool bad = false;
    // im.sums: the two sums adler32 is made of, taken from the symbols as they are decoded — the separate
    // statistics pass over the decoded latent (17 us on a 1080p latent, a tenth of a small image's whole decode) goes away
    unsigned long long s1 = 0, s2 = 0;
    for (uint32_t q = 0; q < blocks; q++) {
        if (loaded < nwords && loaded - min(wpos, loaded) < 4 * 64) {   // top the ring up: the 4 steps below read <= 256 words
            __syncthreads();
            loaded = ring_fill(words, src, loaded, min(nwords, wpos + RING_WORDS), lane);
            __syncthreads();
        }
        uint32_t out4 = 0;
        const int have = (int)min(4u, cnt - min(cnt, q * 256 + lane * 4));   // symbols of this lane in this block
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool active = k < have;
            uint32_t sy, xn;
            if constexpr (BIGTAB) {
                const uint32_t e = big[x & 4095u];
                sy = e & 127u;
                xn = ((e >> 7) & 0x1FFFu) * (x >> PROB_BITS) + (e >> 20);
            } else {
                const uint32_t v = x & 4095u;
                sy = slot[v];
                const uint32_t t = tab.fc[sy];
                xn = (t & 0xFFFFu) * (x >> PROB_BITS) + v - (t >> 16);
            }
            sy = active ? sy : 0u;
            x = active ? xn : x;
            out4 |= sy << (8 * k);
            s1 += sy;
            s2 += (unsigned long long)(n - (begin + q * 256 + lane * 4 + k)) * sy;   // < 2^38 per term, 1024 terms per lane (sy = 0 when inactive)
            const bool need = active && x < RANSW_L;
            const unsigned long long mask = __ballot(need);
            const uint32_t idx = wpos + (uint32_t)__popcll(mask & below);
            const uint32_t wd = words[idx & (RING_WORDS - 1)];   // read unconditionally: no branch on the chain
            bad = bad || (need && idx >= loaded);                // loaded <= nwords; a stream that runs dry is malformed
            x = (need && idx < loaded) ? (x << 16) | wd : x;
            wpos += (uint32_t)__popcll(mask);
        }
        const uint32_t j = q * 256 + lane * 4;
        if (aligned && j + 4 <= cnt)
            *reinterpret_cast<uint32_t *>(lat + begin + j) = out4;
        else
            for (int k = 0; k < 4; k++)
                if (j + k < cnt) lat[begin + j + k] = (uint8_t)(out4 >> (8 * k));
    }
    if (self) {   // this stream's verdict, one plain store
        const unsigned long long any_bad = __ballot(bad || x != RANSW_L || wpos != nwords);
        if (lane == 0) *err = any_bad ? 1u : 0u;
    } else if (bad || x != RANSW_L || wpos != nwords)
        atomicOr(err, 1u);
    unsigned long long *__restrict__ sums = im.sums;
    s2 %= ADLER_MOD;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        s1 += __shfl_down(s1, d);
        s2 += __shfl_down(s2, d);
    }
    if (lane == 0) {
        if (self) {   // per-stream partial sums: a failed stream leaves garbage here, but then the checksum is never looked at
            sums[2 * st] = s1;
            sums[2 * st + 1] = s2 % ADLER_MOD;
        } else {
            if (s1) atomicAdd(&sums[0], s1);
            if (s2) atomicAdd(&sums[1], s2 % ADLER_MOD);
        }
    }
}

// The same without a scan kernel in front (asynchronous encoder, up to SELF_SCAN_MAX streams per image): every workgroup sums
// the lengths of the streams before its own, copies its stream and writes its entry of the container's length table; the last
// one also writes the header's payload-bytes field and the status' byte count (what ransw_scan_body does besides the offsets).
// `cap` = wstream_cap(im.wss), `fixed_bytes` = the container's bytes in front of the payload.
__device__ __forceinline__ void compact_self_body(const EncImage &im, uint32_t st, uint32_t cap, uint32_t fixed_bytes)
{
    const uint8_t *__restrict__ scratch = im.scratch;
    const uint32_t *__restrict__ lens = im.lens;
    uint8_t *__restrict__ out = im.out;
    const uint32_t ns = im.ns;
    uint8_t *table = out + SICN_CODEC_HEADER_BYTES + 256, *payload = table + 4 * (size_t)ns;
    const uint32_t len = lens[st];
    __shared__ uint32_t part[4];
    uint32_t sum = 0;
    for (uint32_t i = threadIdx.x; i < st; i += 256) sum += lens[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    const uint32_t off = part[0] + part[1] + part[2] + part[3];
    const uint8_t *src = scratch + (size_t)st * cap + (cap - len);
    uint8_t *dst = payload + off;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 1) == 0) {   // lengths and offsets are even: 2 bytes at least
        const uint16_t *s2 = reinterpret_cast<const uint16_t *>(src);
        uint16_t *d2 = reinterpret_cast<uint16_t *>(dst);
        for (uint32_t i = threadIdx.x; i < len / 2; i += 256) d2[i] = s2[i];
        if ((len & 1) && threadIdx.x == 0) dst[len - 1] = src[len - 1];
    } else
        for (uint32_t i = threadIdx.x; i < len; i += 256) dst[i] = src[i];
    if (threadIdx.x == 0) {
        uint8_t *p = table + 4 * (size_t)st;
        p[0] = (uint8_t)len; p[1] = (uint8_t)(len >> 8); p[2] = (uint8_t)(len >> 16); p[3] = (uint8_t)(len >> 24);
        if (st == ns - 1) {
            const uint32_t tot = off + len;
            out[40] = (uint8_t)tot; out[41] = (uint8_t)(tot >> 8); out[42] = (uint8_t)(tot >> 16); out[43] = (uint8_t)(tot >> 24);
            im.status[1] = fixed_bytes + tot;   // sicn_codec_status.bytes
        }
    }
}

// The asynchronous decoder's ONLY other stage when the streams were decoded in self mode (ransw_decode_body, self != 0): header,
// frequency table, payload size and length table validated here, AFTER the streams ran (they bound themselves), per-stream
// verdicts and checksum sums folded -> status {error, n_symbols}; the same error bits as dec_parse_body + ransw_scan_body + dec_finish_body.
__device__ __forceinline__ void dec_finish_self_body(const DecImage &im)
{
    const uint8_t *__restrict__ c = im.c;
    const uint32_t *__restrict__ serr = im.err;
    const unsigned long long *__restrict__ ssum = im.sums;
    uint32_t *__restrict__ status = im.status;
    const uint32_t n = im.n, ns = im.ns, lat_w = im.lat_w, lat_h = im.lat_h, lat_c = im.lat_c, wss = im.wss;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t valid = im.valid ? min(*im.valid, im.slot_cap) : im.slot_cap;
    const size_t fixed = SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)ns;
    __shared__ uint32_t r_err, r_tab;
    __shared__ unsigned long long r_s1, r_s2;
    if (tid == 0) { r_err = 0; r_tab = 0; r_s1 = 0; r_s2 = 0; }
    __syncthreads();
    if (valid < fixed) {   // nothing of this slot was read: bit 8 + bit 2, and bit 5 for the streams that all refused it
        if (tid == 0) {
            status[0] = 0x104u | (ns ? 32u : 0u);
            status[1] = n;
        }
        return;
    }
    auto rd32 = [&](size_t o) { return c[o] | ((uint32_t)c[o + 1] << 8) | ((uint32_t)c[o + 2] << 16) | ((uint32_t)c[o + 3] << 24); };
    uint32_t err = 0;
    if (tid < 64) {   // wave 0: the checks of dec_parse_body
        const uint32_t expect[10] = {0x4C434953u, 1u | ((uint32_t)SICN_CODEC_RANSW << 16), 0, 0, lat_w, lat_h, lat_c, n, ns, wss};
        if (lane < 10 && lane != 2 && lane != 3 && rd32(4 * lane) != expect[lane]) err = 4;
        uint32_t fsum = c[SICN_CODEC_HEADER_BYTES + 4 * lane] + ((uint32_t)c[SICN_CODEC_HEADER_BYTES + 4 * lane + 1] << 8) +
                        c[SICN_CODEC_HEADER_BYTES + 4 * lane + 2] + ((uint32_t)c[SICN_CODEC_HEADER_BYTES + 4 * lane + 3] << 8);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) fsum += __shfl_xor((int)fsum, d);
        if (n && fsum != 4096) err |= 8;
    }
    const uint32_t pb = rd32(40);
    const bool pb_bad = (size_t)pb > (size_t)valid - fixed;
    if (tid == 0 && pb_bad) err |= 16;
    const uint32_t bound = pb_bad ? 0u : pb;
    // length table: entries above the cap are an error and count as 0 (scan_body); the per-stream verdicts; the checksum sums
    const uint32_t cap = wstream_cap(wss);
    uint32_t tab = 0;
    unsigned long long s1 = 0, s2 = 0;
    for (uint32_t i = tid; i < ns; i += 256) {
        uint32_t v = rd32(SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)i);
        if (v > cap) { err |= 32; v = 0; }
        tab += v;
        if (serr[i]) err |= 32;
        else { s1 += ssum[2 * i]; s2 += ssum[2 * i + 1]; }
    }
    s2 %= ADLER_MOD;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        err |= (uint32_t)__shfl_xor((int)err, d);
        tab += (uint32_t)__shfl_xor((int)tab, d);
        s1 += __shfl_xor(s1, d);
        s2 += __shfl_xor(s2, d);
    }
    if (lane == 0) {
        if (err) atomicOr(&r_err, err);
        if (tab) atomicAdd(&r_tab, tab);
        if (s1) atomicAdd(&r_s1, s1);
        if (s2) atomicAdd(&r_s2, s2 % ADLER_MOD);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t e = r_err;
        if (r_tab != bound) e |= 64;           // the length table does not add up to the payload
        const uint32_t a = (uint32_t)((1 + r_s1) % ADLER_MOD), b = (uint32_t)((n % ADLER_MOD + r_s2) % ADLER_MOD);
        if (!e && ((b << 16) | a) != rd32(44)) e |= 128;   // checksum (SICN_EBADMSG)
        status[0] = e;
        status[1] = n;
    }
}

// dec_finish_self_body for a WINDOW of the image's streams (k_ragged_window.hip): only the streams [first, end) ran.  The fixed
// part is checked as above — header, frequency table, payload field, every entry of the length table and their sum — the
// per-stream verdicts are folded over [first, end) alone, and the checksum of the whole latent, which a window cannot make, is
// never looked at: bit 7 is never set.  status.bytes = `symbols`, what the selected streams hold.
__device__ __forceinline__ void dec_finish_window_body(const DecImage &im, uint32_t first, uint32_t end, uint32_t symbols)
{
    const uint8_t *__restrict__ c = im.c;
    const uint32_t *__restrict__ serr = im.err;
    uint32_t *__restrict__ status = im.status;
    const uint32_t n = im.n, ns = im.ns, lat_w = im.lat_w, lat_h = im.lat_h, lat_c = im.lat_c, wss = im.wss;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t valid = im.valid ? min(*im.valid, im.slot_cap) : im.slot_cap;
    const size_t fixed = SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)ns;
    __shared__ uint32_t r_err, r_tab;
    if (tid == 0) { r_err = 0; r_tab = 0; }
    __syncthreads();
    if (valid < fixed) {   // nothing of this slot was read: bit 8 + bit 2, and bit 5 for the streams that all refused it
        if (tid == 0) {
            status[0] = 0x104u | (end > first ? 32u : 0u);
            status[1] = symbols;
        }
        return;
    }
    auto rd32 = [&](size_t o) { return c[o] | ((uint32_t)c[o + 1] << 8) | ((uint32_t)c[o + 2] << 16) | ((uint32_t)c[o + 3] << 24); };
    uint32_t err = 0;
    if (tid < 64) {   // wave 0: the checks of dec_parse_body
        const uint32_t expect[10] = {0x4C434953u, 1u | ((uint32_t)SICN_CODEC_RANSW << 16), 0, 0, lat_w, lat_h, lat_c, n, ns, wss};
        if (lane < 10 && lane != 2 && lane != 3 && rd32(4 * lane) != expect[lane]) err = 4;
        uint32_t fsum = c[SICN_CODEC_HEADER_BYTES + 4 * lane] + ((uint32_t)c[SICN_CODEC_HEADER_BYTES + 4 * lane + 1] << 8) +
                        c[SICN_CODEC_HEADER_BYTES + 4 * lane + 2] + ((uint32_t)c[SICN_CODEC_HEADER_BYTES + 4 * lane + 3] << 8);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) fsum += __shfl_xor((int)fsum, d);
        if (n && fsum != 4096) err |= 8;
    }
    const uint32_t pb = rd32(40);
    const bool pb_bad = (size_t)pb > (size_t)valid - fixed;
    if (tid == 0 && pb_bad) err |= 16;
    const uint32_t bound = pb_bad ? 0u : pb;
    const uint32_t cap = wstream_cap(wss);
    uint32_t tab = 0;
    for (uint32_t i = tid; i < ns; i += 256) {
        uint32_t v = rd32(SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)i);
        if (v > cap) { err |= 32; v = 0; }
        tab += v;
        if (i >= first && i < end && serr[i]) err |= 32;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        err |= (uint32_t)__shfl_xor((int)err, d);
        tab += (uint32_t)__shfl_xor((int)tab, d);
    }
    if (lane == 0) {
        if (err) atomicOr(&r_err, err);
        if (tab) atomicAdd(&r_tab, tab);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t e = r_err;
        if (r_tab != bound) e |= 64;           // the length table does not add up to the payload
        status[0] = e;
        status[1] = symbols;
    }
}

// ---- the bookkeeping of the scan form (mode 2, mode 3 above SELF_SCAN_MAX streams, mode 4) --------------------------------------
// First the steps on plain pointers, which mode 2 (one image on the host's schedule) launches as they are; then mode 3's stages of
// one ScanImage.  Mode 4's stages of a CtxImage (k_ctx_body.hpp) are made of the same steps.

// Exclusive prefix sum of `in[0..n)` into out[0..n], out[n] = total.  One workgroup of 1024 lanes:
// wavefront-level scan with __shfl_up, wave totals combined through LDS, carry across chunks.
// `in` may be unaligned container bytes (read byte-wise when `in_bytes` != nullptr).
// Entries above `cap` (only possible in an untrusted container) raise `*err` and count as 0, so with
// n * cap < 2^32 (the n_symbols limit of the rANS modes, MAX_RANS_SYMBOLS) the 32-bit sums cannot wrap.
// skip: a slot the parse stage found shorter than its own fixed part is never read.  status_bytes: sicn_codec_status.bytes or nullptr.
__device__ __forceinline__ void scan_body(const uint32_t *__restrict__ in, const uint8_t *__restrict__ in_bytes, uint32_t n,
                                          uint32_t *__restrict__ out, uint8_t *__restrict__ table_out, uint8_t *__restrict__ total_out,
                                          uint32_t cap, uint32_t *__restrict__ err, uint32_t *__restrict__ status_bytes,
                                          uint32_t fixed_bytes, bool skip)
{
    __shared__ uint32_t wave_tot[16];
    __shared__ uint32_t carry_s;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        uint32_t v = 0;
        if (i < n && !skip) {
            if (in_bytes) {
                const uint8_t *p = in_bytes + 4 * (size_t)i;
                v = p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            } else
                v = in[i];
            if (v > cap) {
                if (err) atomicOr(err, 1u);
                v = 0;
            }
        }
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        if (lane == 63) wave_tot[wv] = incl;
        __syncthreads();
        uint32_t wave_off = 0;
        for (int k = 0; k < wv; k++) wave_off += wave_tot[k];
        const uint32_t carry = carry_s;
        if (i < n) {
            out[i] = carry + wave_off + incl - v;
            if (table_out) {  // the container's per-stream byte counts, little-endian
                uint8_t *p = table_out + 4 * (size_t)i;
                p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
            }
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = carry + wave_off + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t tot = carry_s;
        out[n] = tot;
        if (total_out) {
            total_out[0] = (uint8_t)tot; total_out[1] = (uint8_t)(tot >> 8);
            total_out[2] = (uint8_t)(tot >> 16); total_out[3] = (uint8_t)(tot >> 24);
        }
        if (status_bytes) *status_bytes = fixed_bytes + tot;
    }
}

// one workgroup of 256 per stream: scratch tail -> payload
__device__ __forceinline__ void compact_body(const uint8_t *__restrict__ scratch, const uint32_t *__restrict__ lens,
                                             const uint32_t *__restrict__ offsets, uint8_t *__restrict__ payload, uint32_t cap, uint32_t st)
{
    const uint32_t len = lens[st];
    const uint8_t *src = scratch + (size_t)st * cap + (cap - len);
    uint8_t *dst = payload + offsets[st];
    for (uint32_t i = threadIdx.x; i < len; i += 256) dst[i] = src[i];
}

// the statistics block at the head of a workspace block: hist[256] + sums (64 B) + freq (256 B), then meta (64 B), contiguous
constexpr uint32_t STATS_WORDS = (1024 + 64 + 256) / 4;
// the decoders' parse kernels are the first thing on the stream that touches the workspace: they clear the block themselves
// (one launch less, about 4.5 us of a small image's decode) — everything but meta[0..3], which lane 0 then writes
__device__ __forceinline__ void clear_stats_in_parse(uint32_t *meta, int lane)
{
    uint32_t *h = meta - STATS_WORDS;
    for (uint32_t i = lane; i < STATS_WORDS + 16; i += 64)
        if (i < STATS_WORDS || i >= STATS_WORDS + 4) h[i] = 0;
}

// Decoder back end, ONE lane: stream-level errors, table total, checksum -> status {error, n_symbols}.
__device__ __forceinline__ void dec_finish_body(const uint32_t *__restrict__ meta, const unsigned long long *__restrict__ sums,
                                                const uint32_t *__restrict__ offsets, uint32_t *__restrict__ status, uint32_t n, uint32_t ns)
{
    uint32_t err = meta[0];
    if (meta[3]) err |= 32;                          // a stream overran / underran (the stream decoders, the scan)
    if (offsets[ns] != meta[1]) err |= 64;           // the length table does not add up to the payload
    const uint32_t a = (uint32_t)((1 + sums[0]) % ADLER_MOD), b = (uint32_t)((n % ADLER_MOD + sums[1]) % ADLER_MOD);
    if (!err && ((b << 16) | a) != meta[2]) err |= 128;   // checksum (SICN_EBADMSG)
    status[0] = err;
    status[1] = n;
}

// ---- mode 3, scan form: one image as its bookkeeping stages see it (the stream stages see it as EncImage / DecImage) -----------
struct ScanImage {
    CoderRow r;
    Workspace w;                   // the image's block, carved
    uint8_t *slot;                 // container slot; the decoder only reads it
    const uint32_t *valid;         // decoder: valid bytes of this slot, or nullptr = r.slot_cap
    uint32_t *status;              // sicn_codec_status {error, bytes} of this image
};
// valid: a sicn_codec_status array whose .bytes bound the slots, or nullptr
__device__ __forceinline__ ScanImage scan_image(const CoderRow &r, const uint8_t *containers, const uint32_t *valid, uint32_t *status,
                                                uint8_t *workspace, uint32_t img)
{
    ScanImage im;
    im.r = r;
    carve(im.w, workspace + r.ws_off, r.ns, wstream_cap(r.wss));
    im.slot = const_cast<uint8_t *>(containers) + r.slot_off;
    im.valid = valid ? valid + 2 * (size_t)img + 1 : nullptr;   // sicn_codec_status.bytes
    im.status = status + 2 * (size_t)img;
    return im;
}

// Encoder, one wave, after the statistics: histogram -> 12-bit frequencies (normalize_wave), then the container header and
// frequency table.  status[0] = error flags (bit 0: symbol >= 128, bit 1: normalisation failed).
__device__ __forceinline__ void enc_header_body(const ScanImage &im)
{
    const CoderRow &r = im.r;
    const uint32_t *hist = im.w.hist;
    const int lane = threadIdx.x;
    uint32_t err = 0;
    const uint32_t hh[2] = {hist[2 * lane], hist[2 * lane + 1]};
    if (hist[128 + lane] | hist[192 + lane]) err = 1;
    uint32_t f[2];
    err |= normalize_wave(hh, r.n, f, lane);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) err |= (uint32_t)__shfl_xor((int)err, d);
    if (err) f[0] = f[1] = 0;   // the encode stage skips zero-frequency symbols: it stays memory-safe
    im.w.freq[2 * lane] = (uint16_t)f[0];
    im.w.freq[2 * lane + 1] = (uint16_t)f[1];
    write_header_wave(im.slot, f, im.w.sums[0], im.w.sums[1], r.n, r.ns, r.lat_w, r.lat_h, r.lat_c, r.img_w, r.img_h, r.wss, lane);
    if (lane == 0) im.status[0] = err;
}

// One workgroup of 1024.  Encoder, after the streams: their lengths -> offsets, the container's length table and payload-bytes field,
// status.bytes.  Decoder: the container's length table -> offsets; a slot the parse stage rejected as too short (meta[0] & 0x100) is
// not read: its table counts as empty, and with meta[1] = 0 every stream of it fails its bound off + len <= payload bytes.
__device__ __forceinline__ void ransw_scan_body(const ScanImage &im, bool dec)
{
    uint8_t *table = im.slot + SICN_CODEC_HEADER_BYTES + 256;
    if (dec)
        scan_body(nullptr, table, im.r.ns, im.w.offsets, nullptr, nullptr, wstream_cap(im.r.wss), im.w.meta + 3, nullptr, 0u,
                  (im.w.meta[0] & 0x100u) != 0);
    else
        scan_body(im.w.lens, nullptr, im.r.ns, im.w.offsets, table, im.slot + 40, 0xFFFFFFFFu, nullptr, im.status + 1,
                  (uint32_t)(SICN_CODEC_HEADER_BYTES + 256) + 4 * im.r.ns, false);
}
__device__ __forceinline__ void enc_compact_body(const ScanImage &im, uint32_t st)
{
    compact_body(im.w.scratch, im.w.lens, im.w.offsets, im.slot + SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)im.r.ns,
                 wstream_cap(im.r.wss), st);
}

// Decoder front end, one wave: every header field against the shape the caller expects, the frequency table, and the sizes
// against the bytes the caller vouches for.  meta[0] = error bits, meta[1] = payload bytes the streams may use.
__device__ __forceinline__ void dec_parse_body(const ScanImage &im)
{
    const CoderRow &r = im.r;
    const uint8_t *c = im.slot;
    uint32_t *meta = im.w.meta;
    const int lane = threadIdx.x;
    const uint32_t valid = im.valid ? min(*im.valid, r.slot_cap) : r.slot_cap;
    const size_t fixed = SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)r.ns;
    clear_stats_in_parse(meta, lane);
    if (valid < fixed) {   // nothing of this slot may be read
        if (lane == 0) { meta[0] = 0x104u; meta[1] = 0; meta[2] = 0; meta[3] = 0; }
        return;
    }
    auto rd32 = [&](int o) { return c[o] | ((uint32_t)c[o + 1] << 8) | ((uint32_t)c[o + 2] << 16) | ((uint32_t)c[o + 3] << 24); };
    const uint32_t expect[10] = {0x4C434953u, 1u | ((uint32_t)SICN_CODEC_RANSW << 16), 0, 0, r.lat_w, r.lat_h, r.lat_c, r.n, r.ns, r.wss};
    uint32_t err = 0;
    if (lane < 10 && lane != 2 && lane != 3 && rd32(4 * lane) != expect[lane]) err = 4;
    uint32_t fsum = c[SICN_CODEC_HEADER_BYTES + 4 * lane] + ((uint32_t)c[SICN_CODEC_HEADER_BYTES + 4 * lane + 1] << 8) +
                    c[SICN_CODEC_HEADER_BYTES + 4 * lane + 2] + ((uint32_t)c[SICN_CODEC_HEADER_BYTES + 4 * lane + 3] << 8);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) fsum += __shfl_xor((int)fsum, d);
    if (r.n && fsum != 4096) err |= 8;
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

// Decoder back end of one image, ONE lane
__device__ __forceinline__ void dec_finish_body(const ScanImage &im)
{
    dec_finish_body(im.w.meta, im.w.sums, im.w.offsets, im.status, im.r.n, im.r.ns);
}

}  // namespace
