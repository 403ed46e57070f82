// Latent container + static rANS coder on the GPU (include/sicn_codec.h; specification:
// oracle/sicn_codec_oracle.c).  New functionality: nothing in the reference corresponds to it
// (SURVEY.md §8f rows 1-2), parity status "unpinned".
//
// Two rANS forms.  Mode 3 ("rANS-W") is the wavefront form: a stream of up to 16384 symbols is coded by ONE WAVE, its 64 lanes holding
// 64 interleaved rANS states that share one stream of 16-bit words (stages in k_codec_body.hpp).  Mode 2 is the first, lane-serial
// form, kept for compatibility: streams of 1024 symbols, ONE LANE per stream, every lane writing its stream backwards into a
// fixed-capacity scratch slot; k_rans_scan (wavefront-level prefix scan) turns the sizes into offsets and k_rans_compact copies the streams.
//
// Which entry point runs which launches (mode 3 has ONE host path per direction, the asynchronous pair; both of its forms hand every
// kernel the same base pointers and one UniformBatch):
//   sicn_codec_encode_batch_async[_sl]   up to SELF_SCAN_MAX streams per image, "self" form: k_stats (rows) -> k_ransw_encode (table,
//                                        header and status made by the waves) -> k_compact_self;  above, or with no stream, "scan" form:
//                                        k_clear_stats -> k_stats (atomics) -> k_enc_header -> k_ransw_encode -> k_ransw_scan -> k_enc_compact
//   sicn_codec_decode_batch_async[_sl]   self form: k_ransw_decode<BIGTAB> -> k_dec_finish_self;  scan form: k_dec_parse -> k_ransw_scan ->
//                                        k_ransw_decode<false> -> k_dec_finish
//   sicn_codec_encode_batch, sicn_codec_encode(mode 3)   ransw_encode_sync: the asynchronous encoder + one read-back of the status
//   sicn_codec_decode_batch, sicn_codec_decode(mode 3)   one header read-back (shape, stream length), then ransw_decode_sync: the
//                                        asynchronous decoder + one read-back of the status
//   sicn_codec_encode / _decode, modes 0 - 2   on the host's schedule: k_stats (atomics), host normalize(), k_pack7 / k_unpack7 or
//                                        k_rans_encode -> k_rans_scan -> k_rans_compact / k_rans_scan -> k_rans_decode, k_stats again
//   mode 4 (sicn_codec_ctx.inc)          its own kernels (k_ctx_*) + k_clear_stats and k_stats (atomics) on the statistics block
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/sicn.h"
#include "../../include/sicn_codec.h"
#include "sicn_internal.h"   // chip_geom(): how many waves the device holds decides between the decoder's two table forms

// constants, the workspace layout (carve) and the stages of the rANS-W coder that the ragged kernels (k_ragged_codec.hip) share
#include "k_codec_body.hpp"
// mode 4's constants, workspace layout and stages, shared with k_ragged_ctx.hip
#include "k_ctx_body.hpp"

namespace {

// k_stats grid: at most 128 workgroups per image — each ends with up to 256 global atomics on the SAME 256 words, and those
// serialise in L2.  Measured r02 (tools/coder_speed.py, encode of a 1080p / of 8 4K latents): 32 workgroups 78 / 146 us,
// 128: 80 / 126, 512: 103 / 215.  (Per-workgroup partial histograms summed by the last workgroup to finish were slower
// still: 91 / 203 us — one workgroup walking 128 rows is a serial chain of its own.)
static inline unsigned stats_blocks(uint32_t n) { return std::min((n / 16 + 255u) / 256u + 1u, 128u); }

// ---- kernels ----------------------------------------------------------------------------------
// Batches: blockIdx.y = image.  The rANS-W kernels name their image by a UniformBatch (k_codec_body.hpp), the context coder's by a
// CtxBatch (k_ctx_body.hpp): batch_row() makes the image's row, enc_image() / dec_image() / scan_image() / ctx_image() resolve it to
// pointers, a stage gets the image and blockIdx.x.  Only mode 2, one image on the host's schedule, hands its kernels plain pointers.

// A uniform batch on the host: image 0's row (its offsets are 0: the kernels get the base pointers) and the strides.
// scan = the form without statistics rows (n_rows = 0).  stats_batch: all k_stats needs outside the rANS-W coder (atomic mode on
// the statistics block at the head of a workspace block).
UniformBatch uniform_batch(uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t img_w, uint32_t img_h, uint32_t wss,
                           size_t s_lat, size_t s_slot, size_t s_ws, bool scan)
{
    UniformBatch b{};
    CoderRow &r = b.row0;
    r.n = lat_w * lat_h * lat_c; r.ns = (r.n + wss - 1) / wss; r.wss = wss;
    r.slot_cap = (uint32_t)std::min(s_slot, (size_t)0xFFFFFFFFu);
    r.lat_w = lat_w; r.lat_h = lat_h; r.lat_c = lat_c; r.img_w = img_w; r.img_h = img_h;
    r.n_rows = scan ? 0u : stat_rows(r.n);
    b.s_lat = s_lat; b.s_slot = s_slot; b.s_ws = s_ws;
    b.scan = scan;
    return b;
}
UniformBatch stats_batch(uint32_t n, size_t s_lat, size_t s_ws) { return uniform_batch(n, 1, 1, 0, 0, WSS, s_lat, 0, s_ws, true); }

// histogram (256 bins) + the two sums adler32 is made of (stats_body); scan form: atomics on a cleared block, else one row per workgroup
__global__ __launch_bounds__(256) void k_stats(const uint8_t *__restrict__ latents, uint8_t *__restrict__ workspace, UniformBatch b)
{
    const CoderRow r = batch_row(b);
    Workspace w;
    carve(w, workspace + r.ws_off, r.ns, wstream_cap(r.wss));
    stats_body(latents + r.lat_off, r.n, w.hist, w.sums, b.scan ? nullptr : w.rows + (size_t)blockIdx.x * STAT_ROW_WORDS, blockIdx.x, gridDim.x);
}

// ---- rANS-W: one wave (= one 64-lane workgroup) per stream; the stages are in k_codec_body.hpp ---------------------------
__global__ __launch_bounds__(64) void k_ransw_encode(const uint8_t *__restrict__ latents, uint8_t *__restrict__ containers,
                                                     uint32_t *__restrict__ status, uint8_t *__restrict__ workspace, UniformBatch b)
{
    ransw_encode_body(enc_image(batch_row(b), latents, containers, status, workspace, blockIdx.y, b.scan), blockIdx.x);
}

template <bool BIGTAB>
__global__ __launch_bounds__(64) void k_ransw_decode(const uint8_t *__restrict__ containers, const uint32_t *__restrict__ valid,
                                                     uint8_t *__restrict__ latents, uint8_t *__restrict__ workspace, UniformBatch b)
{
    ransw_decode_body<BIGTAB>(dec_image(batch_row(b), containers, valid, latents, nullptr, workspace, blockIdx.y, b.scan), blockIdx.x, !b.scan);
}


__global__ __launch_bounds__(256) void k_rans_encode(const uint8_t *__restrict__ lat, uint32_t n, uint32_t ns,
                                                     const uint16_t *__restrict__ freq_g, uint8_t *__restrict__ scratch,
                                                     uint32_t *__restrict__ lens)
{
    __shared__ uint16_t freq[128], cum[128];
    if (threadIdx.x < 128) freq[threadIdx.x] = freq_g[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (int s = 0; s < 128; s++) { cum[s] = (uint16_t)c; c += freq[s]; }
    }
    __syncthreads();
    const uint32_t st = blockIdx.x * 256 + threadIdx.x;
    if (st >= ns) return;
    const uint32_t begin = st * SS, cnt = min(SS, n - begin);
    uint8_t *buf = scratch + (size_t)st * CAP;
    uint32_t x = RANS_L, pos = CAP;
    for (uint32_t i = cnt; i-- > 0;) {
        const uint32_t s = lat[begin + i], f = freq[s], c = cum[s];
        const uint32_t x_max = ((RANS_L >> PROB_BITS) << 8) * f;
        while (x >= x_max) {
            buf[--pos] = (uint8_t)(x & 0xFF);
            x >>= 8;
        }
        x = ((x / f) << PROB_BITS) + (x % f) + c;
    }
    buf[--pos] = (uint8_t)(x >> 24);
    buf[--pos] = (uint8_t)(x >> 16);
    buf[--pos] = (uint8_t)(x >> 8);
    buf[--pos] = (uint8_t)x;
    lens[st] = CAP - pos;
}

// Mode 2.  Exclusive prefix sum of a length table by one workgroup of 1024, the arguments as scan_body (k_codec_body.hpp) names them:
// the encoder scans `in` and writes the container's table and payload field, the decoder scans the container's `in_bytes` and has `err`
__global__ __launch_bounds__(1024) void k_rans_scan(const uint32_t *__restrict__ in, const uint8_t *__restrict__ in_bytes, uint32_t n,
                                                    uint32_t *__restrict__ out, uint8_t *__restrict__ table_out,
                                                    uint8_t *__restrict__ total_out, uint32_t cap, uint32_t *__restrict__ err)
{
    scan_body(in, in_bytes, n, out, table_out, total_out, cap, err, nullptr, 0u, false);
}
// one workgroup per stream: scratch tail -> payload
__global__ __launch_bounds__(256) void k_rans_compact(const uint8_t *__restrict__ scratch, const uint32_t *__restrict__ lens,
                                                      const uint32_t *__restrict__ offsets, uint8_t *__restrict__ payload)
{
    compact_body(scratch, lens, offsets, payload, CAP, blockIdx.x);
}

// Mode 3, scan form: the scan of both directions (status: the encoder's; the decoder passes nullptr) and the encoder's compaction
__global__ __launch_bounds__(1024) void k_ransw_scan(const uint8_t *__restrict__ containers, uint32_t *__restrict__ status,
                                                     uint8_t *__restrict__ workspace, UniformBatch b, int dec)
{
    ransw_scan_body(scan_image(batch_row(b), containers, nullptr, status, workspace, blockIdx.y), dec);
}
__global__ __launch_bounds__(256) void k_enc_compact(uint8_t *__restrict__ containers, uint8_t *__restrict__ workspace, UniformBatch b)
{
    enc_compact_body(scan_image(batch_row(b), containers, nullptr, nullptr, workspace, blockIdx.y), blockIdx.x);
}

// The same without a scan kernel in front (asynchronous encoder, up to SELF_SCAN_MAX streams per image): compact_self_body
__global__ __launch_bounds__(256) void k_compact_self(uint8_t *__restrict__ containers, uint32_t *__restrict__ status,
                                                      uint8_t *__restrict__ workspace, UniformBatch b)
{
    const CoderRow r = batch_row(b);
    compact_self_body(enc_image(r, nullptr, containers, status, workspace, blockIdx.y), blockIdx.x, wstream_cap(r.wss),
                      (uint32_t)(SICN_CODEC_HEADER_BYTES + 256) + 4 * r.ns);
}


__global__ __launch_bounds__(256) void k_rans_decode(const uint8_t *__restrict__ payload, const uint8_t *__restrict__ freq_bytes,
                                                     const uint32_t *__restrict__ offsets, uint32_t n, uint32_t ns,
                                                     uint8_t *__restrict__ lat, uint32_t *__restrict__ err, uint32_t payload_bytes)
{
    __shared__ uint16_t freq[128], cum[128];
    __shared__ uint8_t slot[4096];
    if (threadIdx.x < 128) freq[threadIdx.x] = (uint16_t)(freq_bytes[2 * threadIdx.x] | (freq_bytes[2 * threadIdx.x + 1] << 8));
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (int s = 0; s < 128; s++) { cum[s] = (uint16_t)c; c += freq[s]; }
    }
    __syncthreads();
    if (threadIdx.x < 128)
        for (uint32_t v = cum[threadIdx.x]; v < (uint32_t)cum[threadIdx.x] + freq[threadIdx.x] && v < 4096; v++)
            slot[v] = (uint8_t)threadIdx.x;
    __syncthreads();
    const uint32_t st = blockIdx.x * 256 + threadIdx.x;
    if (st >= ns) return;
    const uint32_t begin = st * SS, cnt = min(SS, n - begin);
    if (offsets[st + 1] > payload_bytes || offsets[st + 1] < offsets[st]) { atomicOr(err, 1u); return; }
    const uint8_t *p = payload + offsets[st], *end = payload + offsets[st + 1];
    if (end - p < 4) { atomicOr(err, 1u); return; }
    uint32_t x = p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    p += 4;
    for (uint32_t i = 0; i < cnt; i++) {
        const uint32_t v = x & 4095u, s = slot[v];
        lat[begin + i] = (uint8_t)s;
        x = freq[s] * (x >> PROB_BITS) + v - cum[s];
        while (x < RANS_L) {
            if (p >= end) { atomicOr(err, 1u); return; }
            x = (x << 8) | *p++;
        }
    }
    if (p != end || x != RANS_L) atomicOr(err, 1u);
}

__global__ __launch_bounds__(256) void k_pack7(const uint8_t *__restrict__ lat, uint32_t n, uint8_t *__restrict__ out)
{
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= (n + 7) / 8) return;
    unsigned long long v = 0;
    for (int k = 0; k < 8; k++)
        if (g * 8 + k < n) v |= (unsigned long long)lat[g * 8 + k] << (7 * k);
    for (int k = 0; k < 7; k++) out[7 * (size_t)g + k] = (uint8_t)(v >> (8 * k));
}

__global__ __launch_bounds__(256) void k_unpack7(const uint8_t *__restrict__ in, uint32_t n, uint8_t *__restrict__ lat)
{
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= (n + 7) / 8) return;
    unsigned long long v = 0;
    for (int k = 0; k < 7; k++) v |= (unsigned long long)in[7 * (size_t)g + k] << (8 * k);
    for (int k = 0; k < 8; k++)
        if (g * 8 + k < n) lat[g * 8 + k] = (uint8_t)((v >> (7 * k)) & 127);
}


// ---- asynchronous batch path: everything the host did between two synchronisations, on the device -----------
// The other kernels of mode 3's scan form, one workgroup per image (blockIdx.y); the stages are in k_codec_body.hpp.

// the statistics block at the head of an image's workspace block: the same in mode 3's layout and mode 4's, which passes a stats_batch()
__global__ __launch_bounds__(64) void k_clear_stats(uint8_t *__restrict__ workspace, UniformBatch b)
{
    uint32_t *h = (uint32_t *)(workspace + batch_row(b).ws_off);
    for (uint32_t i = threadIdx.x; i < STATS_WORDS + 16; i += 64) h[i] = 0;
}

__global__ __launch_bounds__(64) void k_enc_header(uint8_t *__restrict__ containers, uint32_t *__restrict__ status,
                                                   uint8_t *__restrict__ workspace, UniformBatch b)
{
    enc_header_body(scan_image(batch_row(b), containers, nullptr, status, workspace, blockIdx.y));
}

__global__ __launch_bounds__(64) void k_dec_parse(const uint8_t *__restrict__ containers, const uint32_t *__restrict__ valid,
                                                  uint8_t *__restrict__ workspace, UniformBatch b)
{
    dec_parse_body(scan_image(batch_row(b), containers, valid, nullptr, workspace, blockIdx.y));
}

// Decoder back end: stream-level errors, table total, checksum -> status {error, n_symbols}.
__global__ __launch_bounds__(64) void k_dec_finish(uint32_t *__restrict__ status, uint8_t *__restrict__ workspace, UniformBatch b)
{
    if (threadIdx.x) return;
    dec_finish_body(scan_image(batch_row(b), nullptr, nullptr, status, workspace, blockIdx.y));
}

// The asynchronous decoder's ONLY other kernel when the streams were decoded in self mode: dec_finish_self_body
__global__ __launch_bounds__(256) void k_dec_finish_self(const uint8_t *__restrict__ containers, const uint32_t *__restrict__ valid,
                                                         uint32_t *__restrict__ status, uint8_t *__restrict__ workspace, UniformBatch b)
{
    dec_finish_self_body(dec_image(batch_row(b), containers, valid, nullptr, status, workspace, blockIdx.y));
}


// ---- host helpers --------------------------------------------------------------------------------
void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
void put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
uint32_t get32(const uint8_t *p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint32_t get16(const uint8_t *p) { return p[0] | ((uint32_t)p[1] << 8); }

// histogram -> 12-bit frequencies; identical to sicl_or_normalize in the oracle's specification
bool normalize(const uint32_t *h, uint32_t n, uint16_t *f)
{
    if (n == 0) return false;
    long long sum = 0;
    for (int s = 0; s < 128; s++) {
        unsigned long long v = h[s] ? ((unsigned long long)h[s] * 4096u) / n : 0;
        if (h[s] && v == 0) v = 1;
        f[s] = (uint16_t)v;
        sum += (long long)v;
    }
    long long diff = 4096 - sum;
    while (diff != 0) {
        int best = -1;
        for (int s = 0; s < 128; s++)
            if (f[s] > 0 && (diff > 0 || f[s] > 1) && (best < 0 || f[s] > f[best])) best = s;
        if (best < 0) return false;
        const long long step = diff > 0 ? diff : (diff < 1 - (long long)f[best] ? 1 - (long long)f[best] : diff);
        f[best] = (uint16_t)((long long)f[best] + step);
        diff -= step;
    }
    return true;
}

uint32_t adler_from_sums(unsigned long long s1, unsigned long long s2, uint32_t n)
{
    const uint32_t a = (uint32_t)((1 + s1) % ADLER_MOD);
    const uint32_t b = (uint32_t)((n % ADLER_MOD + s2) % ADLER_MOD);
    return (b << 16) | a;
}

#define HIP_TRY(x)                         \
    do {                                   \
        if ((x) != hipSuccess) return SICN_ENODEV; \
    } while (0)

}  // namespace

// Host-side exhaustive check of the encoder's divide (the very function the kernel inlines): for every f in
// [f_begin, f_end) and every state the encoder can hold when it divides (x in [2^16, f << 20)), sampled at all
// multiples of f within +-2 of a stride walk, at both ends of the range and around every power of two.
// Returns the number of (x, f) pairs whose quotient or remainder differs from x / f, x % f.
extern "C" long long sicn_codec_selftest_div(uint32_t f_begin, uint32_t f_end, unsigned long long *n_checked)
{
    long long bad = 0;
    unsigned long long cnt = 0;
    for (uint32_t f = f_begin < 1 ? 1 : f_begin; f < f_end && f <= 4096; f++) {
        const uint32_t m = ransw_rcp(f);
        const unsigned long long hi = (unsigned long long)f << 20;        // exclusive
        auto check = [&](unsigned long long xx) {
            if (xx < 65536 || xx >= hi || xx > 0xFFFFFFFFull) return;
            uint32_t r;
            const uint32_t x = (uint32_t)xx, q = ransw_div(x, f, m, r);
            cnt++;
            if (q != x / f || r != x % f) bad++;
        };
        // every 4099th multiple of f (and its neighbours) covers the range with ~256 k..1 M probes per f
        for (unsigned long long k = 65536 / f; k * f < hi + f; k += 4099)
            for (long long d = -2; d <= 2; d++) check(k * f + (unsigned long long)d);
        for (int b = 16; b <= 32; b++)
            for (long long d = -(long long)f - 2; d <= (long long)f + 2; d++) check((1ull << b) + (unsigned long long)d);
        for (long long d = 0; d <= 2 * (long long)f + 2; d++) { check(65536 + d); check(hi - 1 - d); }
    }
    if (n_checked) *n_checked = cnt;
    return bad;
}

// 32-bit stream offsets: ceil(n / wss) scratch slots of wstream_cap(wss) bytes must stay below 2^32 (the static_assert above is
// the 16384 case; 1024-symbol streams allow 1.9 G symbols)
static bool wstream_fits(unsigned long long n, uint32_t wss)
{
    return n <= MAX_RANS_SYMBOLS && ((n + wss - 1) / wss) * (unsigned long long)wstream_cap(wss) < (1ull << 32);
}

extern "C" size_t sicn_codec_max_bytes_sl(uint32_t n, uint32_t wss)
{
    if (!wstream_ok(wss)) return 0;
    const uint32_t ns = (n + wss - 1) / wss;
    return SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)ns + 2 * (size_t)n + 256 * (size_t)ns;
}

extern "C" size_t sicn_codec_workspace_bytes_sl(uint32_t n, uint32_t wss)
{
    if (!wstream_ok(wss)) return 0;
    Workspace w;
    return carve(w, nullptr, (n + wss - 1) / wss, wstream_cap(wss)) + 64;
}

extern "C" size_t sicn_codec_batch_workspace_bytes_sl(uint32_t n_symbols, uint32_t n_images, uint32_t wss)
{
    if (!wstream_ok(wss)) return 0;
    return (size_t)n_images * align_up(sicn_codec_workspace_bytes_sl(n_symbols, wss), 256) + align_up(16 * (size_t)n_images, 256);
}

extern "C" size_t sicn_codec_max_bytes(int mode, uint32_t n)
{
    if (mode == SICN_CODEC_RANSW) return sicn_codec_max_bytes_sl(n, WSS);
    if (mode == SICN_CODEC_RAW8) return SICN_CODEC_HEADER_BYTES + (size_t)n;
    if (mode == SICN_CODEC_PACKED7) return SICN_CODEC_HEADER_BYTES + ((size_t)n + 7) / 8 * 7;
    if (mode == SICN_CODEC_RANS) return SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)((n + SS - 1) / SS) + 2 * (size_t)n + 8 * (size_t)((n + SS - 1) / SS);
    return 0;
}

// Mode 3: per-image blocks, then room for the synchronous wrappers' status arrays (2 x 8 bytes per image) — enough for a
// container of ANY admissible stream length (the synchronous decoders read it from the header)
extern "C" size_t sicn_codec_batch_workspace_bytes(int mode, uint32_t n_symbols, uint32_t n_images)
{
    if (mode != SICN_CODEC_RANSW)
        return (size_t)n_images * align_up(sicn_codec_workspace_bytes(mode, n_symbols), 256) + align_up(16 * (size_t)n_images, 256);
    size_t mx = 0;
    for (uint32_t wss = 1024; wss <= WSS; wss <<= 1)
        if (wstream_fits(n_symbols, wss)) mx = std::max(mx, sicn_codec_batch_workspace_bytes_sl(n_symbols, n_images, wss));
    return mx;
}

extern "C" size_t sicn_codec_workspace_bytes(int mode, uint32_t n)
{
    if (mode == SICN_CODEC_RANSW) return sicn_codec_batch_workspace_bytes(mode, n, 1);   // the synchronous calls are batches of one
    Workspace w;
    return carve(w, nullptr, (n + SS - 1) / SS, mode == SICN_CODEC_RANS ? CAP : 0) + 64;
}

extern "C" int sicn_codec_parse_header(const uint8_t *h, size_t bytes, sicn_codec_info *info)
{
    if (!h || !info || bytes < SICN_CODEC_HEADER_BYTES) return SICN_EINVAL;
    if (std::memcmp(h, "SICL", 4) || get16(h + 4) != 1) return SICN_EINVAL;
    info->mode = get16(h + 6);
    info->image_width = get32(h + 8);
    info->image_height = get32(h + 12);
    info->lat_w = get32(h + 16);
    info->lat_h = get32(h + 20);
    info->lat_c = get32(h + 24);
    info->n_symbols = get32(h + 28);
    info->n_streams = get32(h + 32);
    info->payload_bytes = get32(h + 40);
    info->adler32 = get32(h + 44);
    info->stream_symbols = get32(h + 36);
    if (info->mode > 4) return SICN_EINVAL;
    if (info->mode == SICN_CODEC_RANSW || info->mode == 4 ? !wstream_ok(info->stream_symbols)
                                                          : info->stream_symbols != stream_symbols((int)info->mode))
        return SICN_EINVAL;
    if ((unsigned long long)info->lat_w * info->lat_h * info->lat_c != info->n_symbols) return SICN_EINVAL;
    const uint32_t ss = info->stream_symbols;
    if (info->mode == 4) {   // anchors and non-anchors are cut into streams separately (sicn_codec_ctx.inc)
        const uint32_t W = info->lat_w, H = info->lat_h, C = info->lat_c;
        const unsigned long long na = ((unsigned long long)(H / 2) * W + ((H & 1) ? (W + 1) / 2 : 0)) * C;
        const unsigned long long nn = ((unsigned long long)(H / 2) * W + ((H & 1) ? W / 2 : 0)) * C;
        if (info->n_streams != (na + ss - 1) / ss + (nn + ss - 1) / ss) return SICN_EINVAL;
        return SICN_OK;
    }
    if (info->n_streams != (info->n_symbols + ss - 1) / ss) return SICN_EINVAL;
    return SICN_OK;
}

static int status_to_rc(uint32_t err)
{
    if (!err) return SICN_OK;
    return (err & ~128u) ? SICN_EINVAL : SICN_EBADMSG;
}

// ---- rANS-W: the synchronous calls = the asynchronous pair + one read-back of the status array, which lives behind the
// ---- per-image blocks of the caller's workspace (sicn_codec_batch_workspace_bytes[_sl]) --------------------------
static int ransw_encode_sync(const uint8_t *latents, uint32_t n_images, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint32_t img_w,
                             uint32_t img_h, uint8_t *out, size_t slot_bytes, size_t *out_bytes_host, void *workspace,
                             size_t workspace_bytes, void *hip_stream)
{
    if (!out || !out_bytes_host) return SICN_EINVAL;
    if (n_images == 0) return SICN_OK;
    const unsigned long long n64 = (unsigned long long)lat_w * lat_h * lat_c;
    if (n64 > MAX_RANS_SYMBOLS) return SICN_EINVAL;
    const size_t blocks = (size_t)n_images * align_up(sicn_codec_workspace_bytes_sl((uint32_t)n64, WSS), 256);
    if (!workspace || workspace_bytes < sicn_codec_batch_workspace_bytes(SICN_CODEC_RANSW, (uint32_t)n64, n_images)) return SICN_ENOSPC;
    hipStream_t stream = (hipStream_t)hip_stream;
    sicn_codec_status *st_dev = (sicn_codec_status *)((uint8_t *)workspace + blocks);
    std::vector<sicn_codec_status> st;
    try { st.resize(n_images); } catch (const std::bad_alloc &) { return SICN_ENOMEM; }
    int rc = sicn_codec_encode_batch_async(latents, n_images, lat_w, lat_h, lat_c, img_w, img_h, out, slot_bytes, st_dev, workspace,
                                           workspace_bytes, hip_stream);
    if (rc == SICN_OK && hipMemcpyAsync(st.data(), st_dev, sizeof(sicn_codec_status) * n_images, hipMemcpyDeviceToHost, stream) != hipSuccess)
        rc = SICN_ENODEV;
    if (hipStreamSynchronize(stream) != hipSuccess) return SICN_ENODEV;
    if (rc) return rc;
    for (uint32_t i = 0; i < n_images; i++) {
        if (st[i].error) return SICN_EINVAL;
        out_bytes_host[i] = st[i].bytes;
    }
    return SICN_OK;
}

// n containers of the shape and stream length of `info` (parsed from their headers by the caller), bytes_host[i] valid bytes each
static int ransw_decode_sync(const uint8_t *containers, size_t slot_bytes, const size_t *bytes_host, uint32_t n_images,
                             const sicn_codec_info &info, uint8_t *latents, size_t latent_stride, void *workspace, size_t workspace_bytes,
                             void *hip_stream)
{
    const uint32_t n = info.n_symbols, wss = info.stream_symbols;
    const size_t blocks = (size_t)n_images * align_up(sicn_codec_workspace_bytes_sl(n, wss), 256);
    if (!workspace || workspace_bytes < sicn_codec_batch_workspace_bytes_sl(n, n_images, wss)) return SICN_ENOSPC;
    hipStream_t stream = (hipStream_t)hip_stream;
    std::vector<sicn_codec_status> st;
    try { st.resize(2 * (size_t)n_images); } catch (const std::bad_alloc &) { return SICN_ENOMEM; }
    for (uint32_t i = 0; i < n_images; i++) st[i] = sicn_codec_status{0, (uint32_t)std::min(bytes_host[i], (size_t)0xFFFFFFFFu)};
    sicn_codec_status *st_dev = (sicn_codec_status *)((uint8_t *)workspace + blocks);   // [0, n): valid bytes in, [n, 2n): verdicts out
    int rc = hipMemcpyAsync(st_dev, st.data(), sizeof(sicn_codec_status) * n_images, hipMemcpyHostToDevice, stream) == hipSuccess
                 ? SICN_OK : SICN_ENODEV;
    if (rc == SICN_OK)
        rc = sicn_codec_decode_batch_async_sl(containers, slot_bytes, st_dev, n_images, info.lat_w, info.lat_h, info.lat_c, latents,
                                              latent_stride, st_dev + n_images, workspace, workspace_bytes, hip_stream, wss);
    if (rc == SICN_OK && hipMemcpyAsync(st.data() + n_images, st_dev + n_images, sizeof(sicn_codec_status) * n_images,
                                        hipMemcpyDeviceToHost, stream) != hipSuccess)
        rc = SICN_ENODEV;
    if (hipStreamSynchronize(stream) != hipSuccess) return SICN_ENODEV;
    if (rc) return rc;
    for (uint32_t i = 0; i < n_images; i++)
        if (int e = status_to_rc(st[n_images + i].error)) return e;
    return SICN_OK;
}

// ---- single images: modes 0 - 2 on the host's schedule, mode 3 as a batch of one ---------------------------------
extern "C" int sicn_codec_encode(int mode, const uint8_t *latent, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c,
                                 uint32_t img_w, uint32_t img_h, uint8_t *out, size_t out_capacity, size_t *out_bytes,
                                 void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!out || !out_bytes || mode < 0 || mode > 3) return SICN_EINVAL;
    const unsigned long long n64 = (unsigned long long)lat_w * lat_h * lat_c;
    if (n64 > 0x7fffffffull || (n64 && !latent)) return SICN_EINVAL;
    if (mode >= SICN_CODEC_RANS && n64 > MAX_RANS_SYMBOLS) return SICN_EINVAL;
    const uint32_t n = (uint32_t)n64, ns = (n + SS - 1) / SS;
    if (out_capacity < sicn_codec_max_bytes(mode, n)) return SICN_ENOSPC;
    if (mode == SICN_CODEC_RANSW)   // (slots are even: the bound above is)
        return ransw_encode_sync(latent, 1, lat_w, lat_h, lat_c, img_w, img_h, out, out_capacity & ~(size_t)1, out_bytes, workspace,
                                 workspace_bytes, hip_stream);
    if (!workspace || workspace_bytes < sicn_codec_workspace_bytes(mode, n)) return SICN_ENOSPC;
    hipStream_t stream = (hipStream_t)hip_stream;
    Workspace w;
    carve(w, workspace, ns, mode == SICN_CODEC_RANS ? CAP : 0);

    // statistics (also the checksum and the symbol-range check) -------------------------------
    HIP_TRY(hipMemsetAsync(w.hist, 0, 1024 + 64, stream));
    if (n) hipLaunchKernelGGL(k_stats, dim3(stats_blocks(n)), dim3(256), 0, stream, latent, (uint8_t *)workspace, stats_batch(n, 0, 0));
    uint32_t hist[256];
    unsigned long long sums[2];
    HIP_TRY(hipMemcpyAsync(hist, w.hist, sizeof hist, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(sums, w.sums, sizeof sums, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int s = 128; s < 256; s++)
        if (hist[s]) return SICN_EINVAL;

    uint8_t head[SICN_CODEC_HEADER_BYTES + 256];
    std::memset(head, 0, sizeof head);
    std::memcpy(head, "SICL", 4);
    put16(head + 4, 1);
    put16(head + 6, (uint32_t)mode);
    put32(head + 8, img_w);
    put32(head + 12, img_h);
    put32(head + 16, lat_w);
    put32(head + 20, lat_h);
    put32(head + 24, lat_c);
    put32(head + 28, n);
    put32(head + 32, ns);
    put32(head + 36, SS);
    put32(head + 44, adler_from_sums(sums[0], sums[1], n));

    size_t total;
    if (mode == SICN_CODEC_RAW8) {
        put32(head + 40, n);
        HIP_TRY(hipMemcpyAsync(out, head, SICN_CODEC_HEADER_BYTES, hipMemcpyHostToDevice, stream));
        if (n) HIP_TRY(hipMemcpyAsync(out + SICN_CODEC_HEADER_BYTES, latent, n, hipMemcpyDeviceToDevice, stream));
        total = SICN_CODEC_HEADER_BYTES + (size_t)n;
    } else if (mode == SICN_CODEC_PACKED7) {
        const uint32_t groups = (n + 7) / 8;
        put32(head + 40, groups * 7);
        HIP_TRY(hipMemcpyAsync(out, head, SICN_CODEC_HEADER_BYTES, hipMemcpyHostToDevice, stream));
        if (groups)
            hipLaunchKernelGGL(k_pack7, dim3((groups + 255) / 256), dim3(256), 0, stream, latent, n,
                               out + SICN_CODEC_HEADER_BYTES);
        total = SICN_CODEC_HEADER_BYTES + (size_t)groups * 7;
    } else {
        uint16_t freq[128];
        std::memset(freq, 0, sizeof freq);
        if (n && !normalize(hist, n, freq)) return SICN_EINVAL;
        for (int s = 0; s < 128; s++) put16(head + SICN_CODEC_HEADER_BYTES + 2 * s, freq[s]);
        HIP_TRY(hipMemcpyAsync(out, head, sizeof head, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(w.freq, freq, sizeof freq, hipMemcpyHostToDevice, stream));
        uint8_t *table = out + SICN_CODEC_HEADER_BYTES + 256;
        uint8_t *payload = table + 4 * (size_t)ns;
        if (ns) hipLaunchKernelGGL(k_rans_encode, dim3((ns + 255) / 256), dim3(256), 0, stream, latent, n, ns, w.freq, w.scratch, w.lens);
        hipLaunchKernelGGL(k_rans_scan, dim3(1), dim3(1024), 0, stream, w.lens, nullptr, ns, w.offsets, table, out + 40, 0xFFFFFFFFu, nullptr);
        if (ns) hipLaunchKernelGGL(k_rans_compact, dim3(ns), dim3(256), 0, stream, w.scratch, w.lens, w.offsets, payload);
        uint32_t payload_bytes = 0;
        HIP_TRY(hipMemcpyAsync(&payload_bytes, w.offsets + ns, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        total = SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)ns + payload_bytes;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    if (hipGetLastError() != hipSuccess) return SICN_ENODEV;
    *out_bytes = total;
    return SICN_OK;
}

extern "C" int sicn_codec_decode(const uint8_t *container, size_t bytes, uint8_t *latent, size_t latent_capacity,
                                 sicn_codec_info *info_out, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!container || bytes < SICN_CODEC_HEADER_BYTES) return SICN_EINVAL;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t head[SICN_CODEC_HEADER_BYTES];
    HIP_TRY(hipMemcpyAsync(head, container, sizeof head, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    sicn_codec_info info;
    int rc = sicn_codec_parse_header(head, sizeof head, &info);
    if (rc) return rc;
    if (info_out) *info_out = info;
    const uint32_t n = info.n_symbols, ns = info.n_streams;
    if (n > 0x7fffffffu || (info.mode >= SICN_CODEC_RANS && n > MAX_RANS_SYMBOLS)) return SICN_EINVAL;
    if (n && (!latent || latent_capacity < n)) return SICN_ENOSPC;
    if (info.mode == SICN_CODEC_RANSW) {   // the slot is the caller's bytes (rounded up to the even size slots have; `bytes` bound every read)
        if (!wstream_fits(n, info.stream_symbols)) return SICN_EINVAL;
        return ransw_decode_sync(container, (bytes + 1) & ~(size_t)1, &bytes, 1, info, latent, latent_capacity, workspace, workspace_bytes,
                                 hip_stream);
    }
    if (!workspace || workspace_bytes < sicn_codec_workspace_bytes((int)info.mode, n)) return SICN_ENOSPC;
    Workspace w;
    carve(w, workspace, ns, 0);
    HIP_TRY(hipMemsetAsync(w.hist, 0, 1024 + 64, stream));
    uint32_t *err = w.hist + 255;  // bins >= 128 stay zero for a valid latent: reuse the last one as error flag

    const uint8_t *payload = container + SICN_CODEC_HEADER_BYTES;
    if (info.mode == SICN_CODEC_RAW8) {
        if (info.payload_bytes != n || bytes < SICN_CODEC_HEADER_BYTES + (size_t)n) return SICN_EINVAL;
        if (n) HIP_TRY(hipMemcpyAsync(latent, payload, n, hipMemcpyDeviceToDevice, stream));
    } else if (info.mode == SICN_CODEC_PACKED7) {
        const uint32_t groups = (n + 7) / 8;
        if (info.payload_bytes != groups * 7 || bytes < SICN_CODEC_HEADER_BYTES + (size_t)groups * 7) return SICN_EINVAL;
        if (groups) hipLaunchKernelGGL(k_unpack7, dim3((groups + 255) / 256), dim3(256), 0, stream, payload, n, latent);
    } else {
        const size_t fixed = SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)ns;
        if (bytes < fixed + info.payload_bytes) return SICN_EINVAL;
        const uint8_t *freq_bytes = payload, *table = payload + 256;
        payload = table + 4 * (size_t)ns;
        if (n) {  // the table must sum to 4096 and the stream sizes to payload_bytes
            uint8_t fb[256];
            HIP_TRY(hipMemcpyAsync(fb, freq_bytes, 256, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            uint32_t sum = 0;
            for (int s = 0; s < 128; s++) sum += get16(fb + 2 * s);
            if (sum != 4096) return SICN_EINVAL;
        }
        hipLaunchKernelGGL(k_rans_scan, dim3(1), dim3(1024), 0, stream, nullptr, table, ns, w.offsets, nullptr, nullptr, CAP, err);
        uint32_t total = 0;
        HIP_TRY(hipMemcpyAsync(&total, w.offsets + ns, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (total != info.payload_bytes) return SICN_EINVAL;
        if (ns)
            hipLaunchKernelGGL(k_rans_decode, dim3((ns + 255) / 256), dim3(256), 0, stream, payload, freq_bytes, w.offsets, n, ns, latent, err,
                               info.payload_bytes);
    }
    // checksum of what was decoded
    uint32_t flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, err, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (flag) return SICN_EINVAL;
    HIP_TRY(hipMemsetAsync(w.hist, 0, 1024 + 64, stream));
    if (n) hipLaunchKernelGGL(k_stats, dim3(stats_blocks(n)), dim3(256), 0, stream, latent, (uint8_t *)workspace, stats_batch(n, 0, 0));
    unsigned long long sums[2];
    HIP_TRY(hipMemcpyAsync(sums, w.sums, sizeof sums, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (hipGetLastError() != hipSuccess) return SICN_ENODEV;
    return adler_from_sums(sums[0], sums[1], n) == info.adler32 ? SICN_OK : SICN_EBADMSG;
}


// ---- rANS-W: the asynchronous pair ---------------------------------------------------------------------------
// Everything runs on the device (statistics -> frequency table -> header -> streams -> offsets -> compaction; parse ->
// offsets -> streams -> checksum) and reports through a device status array: no host synchronisation, no allocation,
// capturable in a hipGraph.  Every synchronous rANS-W call is this pair plus the read-back (further down).
extern "C" int sicn_codec_encode_batch_async_sl(const uint8_t *latents, uint32_t n_images, uint32_t lat_w, uint32_t lat_h,
                                                uint32_t lat_c, uint32_t img_w, uint32_t img_h, uint8_t *out, size_t slot_bytes,
                                                sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes,
                                                void *hip_stream, uint32_t wss)
{
    if (!out || !status_dev || !wstream_ok(wss)) return SICN_EINVAL;
    const unsigned long long n64 = (unsigned long long)lat_w * lat_h * lat_c;
    if (!wstream_fits(n64, wss) || (n64 && !latents) || n_images > 65535) return SICN_EINVAL;
    if (n_images == 0) return SICN_OK;
    const uint32_t n = (uint32_t)n64, ns = (n + wss - 1) / wss;
    if (slot_bytes < sicn_codec_max_bytes_sl(n, wss) || (slot_bytes & 1)) return SICN_ENOSPC;
    const size_t ws1 = align_up(sicn_codec_workspace_bytes_sl(n, wss), 256);
    if (!workspace || workspace_bytes < ws1 * n_images) return SICN_ENOSPC;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    uint32_t *status = (uint32_t *)status_dev;
    const bool scan = ns == 0 || ns > SELF_SCAN_MAX;
    const UniformBatch b = uniform_batch(lat_w, lat_h, lat_c, img_w, img_h, wss, n, slot_bytes, ws1, scan);
    if (!scan) {
        // three launches (round 4; four in round 3, six in round 2): statistics in rows (no clear, no atomics) -> streams, every
        // wave making the frequency table from the rows itself and stream 0's wave writing header, table and status ->
        // compaction with its own scan
        hipLaunchKernelGGL(k_stats, dim3(b.row0.n_rows, n_images), dim3(256), 0, stream, latents, ws, b);
        hipLaunchKernelGGL(k_ransw_encode, dim3(ns, n_images), dim3(64), 0, stream, latents, out, status, ws, b);
        hipLaunchKernelGGL(k_compact_self, dim3(ns, n_images), dim3(256), 0, stream, out, status, ws, b);
        return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
    }
    hipLaunchKernelGGL(k_clear_stats, dim3(1, n_images), dim3(64), 0, stream, ws, b);
    if (n) hipLaunchKernelGGL(k_stats, dim3(stats_blocks(n), n_images), dim3(256), 0, stream, latents, ws, b);
    hipLaunchKernelGGL(k_enc_header, dim3(1, n_images), dim3(64), 0, stream, out, status, ws, b);
    if (ns) hipLaunchKernelGGL(k_ransw_encode, dim3(ns, n_images), dim3(64), 0, stream, latents, out, status, ws, b);
    hipLaunchKernelGGL(k_ransw_scan, dim3(1, n_images), dim3(1024), 0, stream, out, status, ws, b, 0);
    if (ns) hipLaunchKernelGGL(k_enc_compact, dim3(ns, n_images), dim3(256), 0, stream, out, ws, b);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_codec_encode_batch_async(const uint8_t *latents, uint32_t n_images, uint32_t lat_w, uint32_t lat_h,
                                             uint32_t lat_c, uint32_t img_w, uint32_t img_h, uint8_t *out, size_t slot_bytes,
                                             sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes,
                                             void *hip_stream)
{
    return sicn_codec_encode_batch_async_sl(latents, n_images, lat_w, lat_h, lat_c, img_w, img_h, out, slot_bytes, status_dev, workspace,
                                            workspace_bytes, hip_stream, WSS);
}

extern "C" int sicn_codec_decode_batch_async_sl(const uint8_t *containers, size_t slot_bytes, const sicn_codec_status *valid_dev_or_null,
                                                uint32_t n_images, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint8_t *latents,
                                                size_t latent_stride, sicn_codec_status *status_dev, void *workspace,
                                                size_t workspace_bytes, void *hip_stream, uint32_t wss)
{
    if (!containers || !status_dev || (slot_bytes & 1) || !wstream_ok(wss)) return SICN_EINVAL;
    const unsigned long long n64 = (unsigned long long)lat_w * lat_h * lat_c;
    if (!wstream_fits(n64, wss) || n_images > 65535) return SICN_EINVAL;
    if (n_images == 0) return SICN_OK;
    const uint32_t n = (uint32_t)n64, ns = (n + wss - 1) / wss;
    if (n && (!latents || latent_stride < n)) return SICN_ENOSPC;
    const size_t ws1 = align_up(sicn_codec_workspace_bytes_sl(n, wss), 256);
    if (!workspace || workspace_bytes < ws1 * n_images) return SICN_ENOSPC;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *ws = (uint8_t *)workspace;
    const uint32_t *valid = (const uint32_t *)valid_dev_or_null;
    const bool scan = ns > SELF_SCAN_MAX;
    const UniformBatch b = uniform_batch(lat_w, lat_h, lat_c, 0, 0, wss, latent_stride, slot_bytes, ws1, scan);
    if (!scan) {
        // two launches instead of four: the streams bound and place themselves (self mode), the finish kernel validates header
        // and table and folds the per-stream verdicts / checksum sums (a small image's decode is mostly launch latency)
        if (ns) {
            // the latency form (one 16 KB table, one LDS round trip less per step) while all waves of the batch fit the chip at
            // five per CU; beyond that the two-table form, whose lookups the other eleven waves of a CU hide
            sicn::ChipGeom chip;
            const bool big = sicn::chip_geom(&chip) == SICN_OK && (unsigned long long)ns * n_images <= 5ull * (unsigned)chip.n_cu;
            if (big)
                hipLaunchKernelGGL(k_ransw_decode<true>, dim3(ns, n_images), dim3(64), 0, stream, containers, valid, latents, ws, b);
            else
                hipLaunchKernelGGL(k_ransw_decode<false>, dim3(ns, n_images), dim3(64), 0, stream, containers, valid, latents, ws, b);
        }
        hipLaunchKernelGGL(k_dec_finish_self, dim3(1, n_images), dim3(256), 0, stream, containers, valid, (uint32_t *)status_dev, ws, b);
        return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
    }
    hipLaunchKernelGGL(k_dec_parse, dim3(1, n_images), dim3(64), 0, stream, containers, valid, ws, b);
    hipLaunchKernelGGL(k_ransw_scan, dim3(1, n_images), dim3(1024), 0, stream, containers, (uint32_t *)nullptr, ws, b, 1);
    hipLaunchKernelGGL(k_ransw_decode<false>, dim3(ns, n_images), dim3(64), 0, stream, containers, valid, latents, ws, b);
    hipLaunchKernelGGL(k_dec_finish, dim3(1, n_images), dim3(64), 0, stream, (uint32_t *)status_dev, ws, b);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_codec_decode_batch_async(const uint8_t *containers, size_t slot_bytes, const sicn_codec_status *valid_dev_or_null,
                                             uint32_t n_images, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, uint8_t *latents,
                                             size_t latent_stride, sicn_codec_status *status_dev, void *workspace,
                                             size_t workspace_bytes, void *hip_stream)
{
    return sicn_codec_decode_batch_async_sl(containers, slot_bytes, valid_dev_or_null, n_images, lat_w, lat_h, lat_c, latents,
                                            latent_stride, status_dev, workspace, workspace_bytes, hip_stream, WSS);
}

extern "C" int sicn_codec_encode_batch(int mode, const uint8_t *latents, uint32_t n_images, uint32_t lat_w, uint32_t lat_h,
                                       uint32_t lat_c, uint32_t img_w, uint32_t img_h, uint8_t *out, size_t slot_bytes,
                                       size_t *out_bytes_host, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (mode != SICN_CODEC_RANSW) return SICN_EINVAL;
    return ransw_encode_sync(latents, n_images, lat_w, lat_h, lat_c, img_w, img_h, out, slot_bytes, out_bytes_host, workspace,
                             workspace_bytes, hip_stream);
}

extern "C" int sicn_codec_decode_batch(const uint8_t *containers, size_t slot_bytes, const size_t *bytes_host, uint32_t n_images,
                                       uint8_t *latents, size_t latent_stride, sicn_codec_info *infos_or_null, void *workspace,
                                       size_t workspace_bytes, void *hip_stream)
{
    if (!containers || !bytes_host || (slot_bytes & 1)) return SICN_EINVAL;
    if (n_images == 0) return SICN_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    std::vector<uint8_t> head;
    std::vector<sicn_codec_info> info;
    try {
        head.resize((size_t)n_images * SICN_CODEC_HEADER_BYTES);
        info.resize(n_images);
    } catch (const std::bad_alloc &) { return SICN_ENOMEM; }
    // first synchronisation: the shape comes out of the containers (the async entry point takes it from the caller)
    for (uint32_t i = 0; i < n_images; i++) {
        if (bytes_host[i] < SICN_CODEC_HEADER_BYTES + 256 || bytes_host[i] > slot_bytes) return SICN_EINVAL;
        HIP_TRY(hipMemcpyAsync(&head[(size_t)i * SICN_CODEC_HEADER_BYTES], containers + (size_t)i * slot_bytes, SICN_CODEC_HEADER_BYTES,
                               hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    for (uint32_t i = 0; i < n_images; i++) {
        int rc = sicn_codec_parse_header(&head[(size_t)i * SICN_CODEC_HEADER_BYTES], SICN_CODEC_HEADER_BYTES, &info[i]);
        if (rc) return rc;
        if (info[i].mode != SICN_CODEC_RANSW) return SICN_EINVAL;
        if (info[i].lat_w != info[0].lat_w || info[i].lat_h != info[0].lat_h || info[i].lat_c != info[0].lat_c) return SICN_EINVAL;
        if (info[i].stream_symbols != info[0].stream_symbols) return SICN_EINVAL;   // one batch = one stream length
        if (info[i].n_symbols > MAX_RANS_SYMBOLS) return SICN_EINVAL;
        if (infos_or_null) infos_or_null[i] = info[i];
    }
    return ransw_decode_sync(containers, slot_bytes, bytes_host, n_images, info[0], latents, latent_stride, workspace, workspace_bytes,
                             hip_stream);
}

#include "sicn_codec_ctx.inc"   // container mode 4: class-conditional rANS-W with a checkerboard context model
