// Latent container + static rANS coder on the GPU (include/sicn_codec.h; specification:
// oracle/sicn_codec_oracle.c).  New functionality: nothing in the reference corresponds to it
// (SURVEY.md §8f rows 1-2), parity status "unpinned".
//
// Two rANS forms.  Mode 3 ("rANS-W") is the wavefront form: a stream of 16384 symbols is coded by ONE
// WAVE, its 64 lanes holding 64 interleaved rANS states that share one stream of 16-bit words; in every
// step each lane codes one symbol and the lanes that renormalise find their word by a wavefront-level
// scan of one ballot (rank = popcount of the emitting lanes below).  Symbols are read and written 64
// consecutive bytes at a time.  Mode 2 is the first, lane-serial form, kept for compatibility:
// the latent is cut into independent streams of 1024 symbols; ONE LANE encodes or
// decodes one stream (rANS is inherently serial inside a stream), so a 4K latent (6.2 M symbols)
// is 6 075 lanes.  Stream sizes are data dependent: every lane writes its stream backwards into a
// fixed-capacity scratch slot, a wavefront-level prefix scan (k_scan: __shfl_up inside a wave,
// LDS across the 16 waves of one workgroup, running carry across chunks) turns the sizes into
// offsets, and a copy kernel compacts the streams into the container.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/sicn.h"
#include "../../include/sicn_codec.h"
#include "sicn_internal.h"   // chip_geom(): how many waves the device holds decides between the decoder's two table forms

// constants, the workspace layout (carve) and the stages of the rANS-W coder that the ragged kernels (k_ragged_codec.hip) share
#include "k_codec_body.hpp"

namespace {

// k_stats grid: at most 128 workgroups per image — each ends with up to 256 global atomics on the SAME 256 words, and those
// serialise in L2.  Measured r02 (tools/coder_speed.py, encode of a 1080p / of 8 4K latents): 32 workgroups 78 / 146 us,
// 128: 80 / 126, 512: 103 / 215.  (Per-workgroup partial histograms summed by the last workgroup to finish were slower
// still: 91 / 203 us — one workgroup walking 128 rows is a serial chain of its own.)
static inline unsigned stats_blocks(uint32_t n, uint32_t n_images)
{
    (void)n_images;
    return std::min((n / 16 + 255u) / 256u + 1u, 128u);
}

// ---- kernels ----------------------------------------------------------------------------------
// histogram (256 bins) + the two sums adler32 is made of; grid-stride over 16-byte groups (consecutive lanes read
// consecutive groups); zeros — half of a ReLU latent — are counted in a register instead of hammering one LDS bin
// Batches: blockIdx.y = image; pointers into the latent tensor / the per-image workspace / the container
// slots advance by the given byte strides (0 for single-image calls).
template <typename T>
__device__ __forceinline__ T *img_ptr(T *p, size_t stride)
{
    return (T *)((uint8_t *)p + (size_t)blockIdx.y * stride);
}
template <typename T>
__device__ __forceinline__ const T *img_ptr(const T *p, size_t stride)
{
    return (const T *)((const uint8_t *)p + (size_t)blockIdx.y * stride);
}

__global__ __launch_bounds__(256) void k_stats(const uint8_t *__restrict__ lat_, uint32_t n, uint32_t *__restrict__ hist_,
                                               unsigned long long *__restrict__ sums_, size_t s_lat, size_t s_ws,
                                               uint32_t *__restrict__ rows_ = nullptr)
{
    stats_body(img_ptr(lat_, s_lat), n, img_ptr(hist_, s_ws), img_ptr(sums_, s_ws),
               rows_ ? img_ptr(rows_, s_ws) + (size_t)blockIdx.x * STAT_ROW_WORDS : nullptr, blockIdx.x, gridDim.x);
}

// ---- rANS-W: one wave (= one 64-lane workgroup) per stream; the stages are in k_codec_body.hpp ---------------------------
// what the asynchronous encoder's streams need to make the frequency table THEMSELVES from the statistics rows (row mode)
struct EncSelfHeader {
    const uint32_t *rows;     // [n_rows][STAT_ROW_WORDS] per image (stride s_ws), or nullptr: the table comes from freq_g
    uint32_t n_rows;
    uint8_t *out;             // containers (stride s_slot)
    size_t s_slot;
    uint32_t *status;         // sicn_codec_status[n_images]
    uint32_t lat_w, lat_h, lat_c, img_w, img_h;
};

__global__ __launch_bounds__(64) void k_ransw_encode(const uint8_t *__restrict__ lat_, uint32_t n, uint32_t ns,
                                                     const uint16_t *__restrict__ freq_g_, uint8_t *__restrict__ scratch_,
                                                     uint32_t *__restrict__ lens_, size_t s_lat, size_t s_ws, uint32_t wss,
                                                     EncSelfHeader sh = EncSelfHeader{})
{
    EncImage im;
    im.lat = img_ptr(lat_, s_lat);
    im.n = n; im.ns = ns; im.wss = wss;
    im.scratch = img_ptr(scratch_, s_ws);
    im.lens = img_ptr(lens_, s_ws);
    im.rows = sh.rows ? img_ptr(sh.rows, s_ws) : nullptr;
    im.freq = img_ptr(freq_g_, s_ws);
    im.n_rows = sh.n_rows;
    im.out = img_ptr(sh.out, sh.s_slot);
    im.status = sh.status + 2 * blockIdx.y;
    im.lat_w = sh.lat_w; im.lat_h = sh.lat_h; im.lat_c = sh.lat_c; im.img_w = sh.img_w; im.img_h = sh.img_h;
    ransw_encode_body(im, blockIdx.x);
}

template <bool BIGTAB>
__global__ __launch_bounds__(64) void k_ransw_decode(const uint8_t *__restrict__ payload_, const uint8_t *__restrict__ freq_bytes_,
                                                     const uint32_t *__restrict__ offsets_, uint32_t n, uint32_t ns,
                                                     uint8_t *__restrict__ lat_, uint32_t *__restrict__ err_, size_t s_slot,
                                                     size_t s_ws, size_t s_lat, const uint8_t *__restrict__ payload_bytes_field_,
                                                     const uint32_t *__restrict__ meta_, unsigned long long *__restrict__ sums_, uint32_t wss,
                                                     const uint32_t *__restrict__ self_valid_ = nullptr, uint32_t self_valid_stride = 0,
                                                     int self = 0)
{
    DecImage im;
    im.c = nullptr;
    im.pbf = img_ptr(payload_bytes_field_, s_slot);
    im.freq_bytes = img_ptr(freq_bytes_, s_slot);
    im.payload = img_ptr(payload_, s_slot);
    im.slot_cap = (uint32_t)min(s_slot, (size_t)0xFFFFFFFFu);
    im.valid = self_valid_ ? self_valid_ + (size_t)blockIdx.y * self_valid_stride : nullptr;
    im.lat = img_ptr(lat_, s_lat);
    im.n = n; im.ns = ns; im.wss = wss;
    im.lat_w = im.lat_h = im.lat_c = 0;
    im.err = img_ptr(err_, s_ws);
    im.sums = sums_ ? img_ptr(sums_, s_ws) : nullptr;
    im.offsets = img_ptr(offsets_, s_ws);
    im.meta = meta_ ? img_ptr(meta_, s_ws) : nullptr;
    im.status = nullptr;
    ransw_decode_body<BIGTAB>(im, blockIdx.x, self);
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

// Exclusive prefix sum of `in[0..n)` into out[0..n], out[n] = total.  One workgroup of 1024 lanes:
// wavefront-level scan with __shfl_up, wave totals combined through LDS, carry across chunks.
// `in` may be unaligned container bytes (read byte-wise when `in_bytes` != nullptr).
// Entries above `cap` (only possible in an untrusted container) raise `*err` and count as 0, so with
// n * cap < 2^32 (the n_symbols limit of the rANS modes, MAX_RANS_SYMBOLS) the 32-bit sums cannot wrap.
__global__ __launch_bounds__(1024) void k_scan(const uint32_t *__restrict__ in_, const uint8_t *__restrict__ in_bytes_,
                                               uint32_t n, uint32_t *__restrict__ out_, uint8_t *__restrict__ table_out_,
                                               uint8_t *__restrict__ total_out_, size_t s_ws, size_t s_slot, uint32_t cap,
                                               uint32_t *__restrict__ err_, uint32_t *__restrict__ status_bytes_ = nullptr,
                                               uint32_t fixed_bytes = 0, const uint32_t *__restrict__ skip_meta_ = nullptr)
{
    // async decode: a slot the parse stage found shorter than its own fixed part (meta[0] & 0x100) is never read
    const bool skip = skip_meta_ && (img_ptr(skip_meta_, s_ws)[0] & 0x100u);
    const uint32_t *in = in_ ? img_ptr(in_, s_ws) : nullptr;
    const uint8_t *in_bytes = in_bytes_ ? img_ptr(in_bytes_, s_slot) : nullptr;
    uint32_t *out = img_ptr(out_, s_ws);
    uint8_t *table_out = table_out_ ? img_ptr(table_out_, s_slot) : nullptr;
    uint8_t *total_out = total_out_ ? img_ptr(total_out_, s_slot) : nullptr;
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
                if (err_) atomicOr(img_ptr(err_, s_ws), 1u);
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
        if (status_bytes_) status_bytes_[2 * blockIdx.y + 1] = fixed_bytes + tot;   // sicn_codec_status.bytes
    }
}

// one workgroup per stream: scratch tail -> payload
__global__ __launch_bounds__(256) void k_compact(const uint8_t *__restrict__ scratch_, const uint32_t *__restrict__ lens_,
                                                 const uint32_t *__restrict__ offsets_, uint8_t *__restrict__ payload_, uint32_t cap,
                                                 size_t s_ws, size_t s_slot)
{
    const uint8_t *scratch = img_ptr(scratch_, s_ws);
    const uint32_t *lens = img_ptr(lens_, s_ws), *offsets = img_ptr(offsets_, s_ws);
    uint8_t *payload = img_ptr(payload_, s_slot);
    const uint32_t st = blockIdx.x, len = lens[st];
    const uint8_t *src = scratch + (size_t)st * cap + (cap - len);
    uint8_t *dst = payload + offsets[st];
    for (uint32_t i = threadIdx.x; i < len; i += 256) dst[i] = src[i];
}

// The same without a scan kernel in front (asynchronous encoder, up to SELF_SCAN_MAX streams per image): compact_self_body
__global__ __launch_bounds__(256) void k_compact_self(const uint8_t *__restrict__ scratch_, const uint32_t *__restrict__ lens_,
                                                      uint8_t *__restrict__ out_, uint32_t cap, uint32_t ns, size_t s_ws, size_t s_slot,
                                                      uint32_t *__restrict__ status_bytes_, uint32_t fixed_bytes)
{
    EncImage im{};
    im.scratch = const_cast<uint8_t *>(img_ptr(scratch_, s_ws));
    im.lens = const_cast<uint32_t *>(img_ptr(lens_, s_ws));
    im.ns = ns;
    im.out = img_ptr(out_, s_slot);
    im.status = status_bytes_ + 2 * blockIdx.y;
    compact_self_body(im, blockIdx.x, cap, fixed_bytes);
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
// blockIdx.y = image everywhere; per-image workspace stride s_ws, container slot stride s_slot.

constexpr uint32_t STATS_WORDS = (1024 + 64 + 256) / 4;   // hist[256] + sums (64 B) + freq (256 B), then meta (64 B): contiguous
__global__ __launch_bounds__(64) void k_clear_stats(uint32_t *__restrict__ hist_, size_t s_ws)
{
    uint32_t *h = img_ptr(hist_, s_ws);
    for (uint32_t i = threadIdx.x; i < STATS_WORDS + 16; i += 64) h[i] = 0;
}
// the decoders' parse kernels are the first thing on the stream that touches the workspace: they clear the block themselves
// (one launch less, about 4.5 us of a small image's decode) — everything but meta[0..3], which lane 0 then writes
__device__ __forceinline__ void clear_stats_in_parse(uint32_t *meta, int lane)
{
    uint32_t *h = meta - STATS_WORDS;
    for (uint32_t i = lane; i < STATS_WORDS + 16; i += 64)
        if (i < STATS_WORDS || i >= STATS_WORDS + 4) h[i] = 0;
}

// Histogram -> 12-bit frequencies exactly as `normalize` / sicl_or_normalize do it (same floor, same "largest first,
// lowest index on ties" correction walk), by one wave: lane l owns symbols 2l, 2l+1.  Then the container header and
// frequency table.  status[0] = error flags (bit 0: symbol >= 128, bit 1: normalisation failed).
__global__ __launch_bounds__(256) void k_enc_header(const uint32_t *__restrict__ hist_, const unsigned long long *__restrict__ sums_,
                                                   uint16_t *__restrict__ freq_, uint8_t *__restrict__ out_, uint32_t *__restrict__ status_,
                                                   uint32_t n, uint32_t ns, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c,
                                                   uint32_t img_w, uint32_t img_h, size_t s_ws, size_t s_slot, uint32_t wss,
                                                   const uint32_t *__restrict__ rows_ = nullptr, uint32_t n_rows = 0)
{
    const uint32_t *hist = img_ptr(hist_, s_ws);
    const unsigned long long *sums = img_ptr(sums_, s_ws);
    uint16_t *freq = img_ptr(freq_, s_ws);
    uint8_t *out = img_ptr(out_, s_slot);
    uint32_t *status = status_ + 2 * blockIdx.y;
    const int lane = threadIdx.x;
    uint32_t err = 0;
    uint32_t hh[2], hi = 0;
    unsigned long long s1 = 0, s2 = 0;
    if (rows_) {   // row mode (launched with 4 waves): the statistics workgroups' rows are summed here, wave w = rows w, w + 4, ..
        const uint32_t *rows = img_ptr(rows_, s_ws);
        __shared__ uint32_t part[4][260];
        const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        unsigned long long p1 = 0, p2 = 0;
#pragma unroll 4
        for (uint32_t r = wv; r < n_rows; r += 4) {
            const uint32_t *row = rows + (size_t)r * STAT_ROW_WORDS;
            a0 += row[l];
            a1 += row[64 + l];
            a2 += row[128 + l];
            a3 += row[192 + l];
            if (l == 0) {
                const unsigned long long *q = (const unsigned long long *)(row + 256);
                p1 += q[0];
                p2 += q[1];
            }
        }
        part[wv][l] = a0; part[wv][64 + l] = a1; part[wv][128 + l] = a2; part[wv][192 + l] = a3;
        if (l == 0) {
            part[wv][256] = (uint32_t)p1; part[wv][257] = (uint32_t)(p1 >> 32);
            part[wv][258] = (uint32_t)p2; part[wv][259] = (uint32_t)(p2 >> 32);
        }
        __syncthreads();
        if (wv) return;
        auto tot = [&](int i) { return part[0][i] + part[1][i] + part[2][i] + part[3][i]; };
        hh[0] = tot(2 * lane);
        hh[1] = tot(2 * lane + 1);
        hi = tot(128 + lane) | tot(192 + lane);
        for (int k = 0; k < 4; k++) {
            s1 += part[k][256] | ((unsigned long long)part[k][257] << 32);
            s2 += part[k][258] | ((unsigned long long)part[k][259] << 32);
        }
    } else {
        hh[0] = hist[2 * lane];
        hh[1] = hist[2 * lane + 1];
        hi = hist[128 + lane] | hist[192 + lane];
        s1 = sums[0];
        s2 = sums[1];
    }
    if (hi) err = 1;
    uint32_t f[2];
    err |= normalize_wave(hh, n, f, lane);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) err |= (uint32_t)__shfl_xor((int)err, d);
    if (err) f[0] = f[1] = 0;   // the encode kernel skips zero-frequency symbols: it stays memory-safe
    freq[2 * lane] = (uint16_t)f[0];
    freq[2 * lane + 1] = (uint16_t)f[1];
    write_header_wave(out, f, s1, s2, n, ns, lat_w, lat_h, lat_c, img_w, img_h, wss, lane);
    if (lane == 0) status[0] = err;
}

// Decoder front end: every header field against the shape the caller expects, the frequency table, and the sizes
// against the bytes the caller vouches for.  meta[0] |= error bits, meta[1] = payload bytes the streams may use.
__global__ __launch_bounds__(64) void k_dec_parse(const uint8_t *__restrict__ containers_, const uint32_t *__restrict__ valid_bytes_,
                                                  uint32_t valid_stride, uint32_t *__restrict__ meta_, uint32_t n, uint32_t ns,
                                                  uint32_t lat_w, uint32_t lat_h, uint32_t lat_c, size_t s_slot, size_t s_ws, uint32_t wss)
{
    const uint8_t *c = img_ptr(containers_, s_slot);
    uint32_t *meta = img_ptr(meta_, s_ws);
    const int lane = threadIdx.x;
    const uint32_t valid = valid_bytes_ ? min(valid_bytes_[(size_t)blockIdx.y * valid_stride], (uint32_t)min(s_slot, (size_t)0xFFFFFFFFu))
                                        : (uint32_t)min(s_slot, (size_t)0xFFFFFFFFu);
    const size_t fixed = SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)ns;
    uint32_t err = 0;
    clear_stats_in_parse(meta, lane);
    if (valid < fixed) {   // nothing of this slot may be read
        if (lane == 0) { meta[0] = 0x104u; meta[1] = 0; meta[2] = 0; meta[3] = 0; }
        return;
    }
    auto rd32 = [&](int o) { return c[o] | ((uint32_t)c[o + 1] << 8) | ((uint32_t)c[o + 2] << 16) | ((uint32_t)c[o + 3] << 24); };
    const uint32_t expect[10] = {0x4C434953u, 1u | ((uint32_t)SICN_CODEC_RANSW << 16), 0, 0, lat_w, lat_h, lat_c, n, ns, wss};
    if (lane < 10 && lane != 2 && lane != 3 && rd32(4 * lane) != expect[lane]) err = 4;
    uint32_t fsum = c[SICN_CODEC_HEADER_BYTES + 4 * lane] + ((uint32_t)c[SICN_CODEC_HEADER_BYTES + 4 * lane + 1] << 8) +
                    c[SICN_CODEC_HEADER_BYTES + 4 * lane + 2] + ((uint32_t)c[SICN_CODEC_HEADER_BYTES + 4 * lane + 3] << 8);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) fsum += __shfl_xor((int)fsum, d);
    if (n && fsum != 4096) err |= 8;
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

// Decoder back end: stream-level errors, table total, checksum -> status {error, n_symbols}.
__global__ __launch_bounds__(64) void k_dec_finish(const uint32_t *__restrict__ meta_, const uint32_t *__restrict__ hist_,
                                                   const unsigned long long *__restrict__ sums_, const uint32_t *__restrict__ offsets_,
                                                   uint32_t *__restrict__ status_, uint32_t n, uint32_t ns, size_t s_ws)
{
    if (threadIdx.x) return;
    const uint32_t *meta = img_ptr(meta_, s_ws), *offsets = img_ptr(offsets_, s_ws);
    (void)hist_;
    const unsigned long long *sums = img_ptr(sums_, s_ws);
    uint32_t err = meta[0];
    if (meta[3]) err |= 32;                          // a stream overran / underran (k_ransw_decode, k_scan)
    if (offsets[ns] != meta[1]) err |= 64;           // the length table does not add up to the payload
    const uint32_t a = (uint32_t)((1 + sums[0]) % ADLER_MOD), b = (uint32_t)((n % ADLER_MOD + sums[1]) % ADLER_MOD);
    if (!err && ((b << 16) | a) != meta[2]) err |= 128;   // checksum (SICN_EBADMSG)
    status_[2 * blockIdx.y] = err;
    status_[2 * blockIdx.y + 1] = n;
}

// The asynchronous decoder's ONLY other kernel when the streams were decoded in self mode: dec_finish_self_body
__global__ __launch_bounds__(256) void k_dec_finish_self(const uint8_t *__restrict__ containers_, const uint32_t *__restrict__ valid_bytes_,
                                                         uint32_t valid_stride, const uint32_t *__restrict__ serr_,
                                                         const unsigned long long *__restrict__ ssum_, uint32_t *__restrict__ status_,
                                                         uint32_t n, uint32_t ns, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c,
                                                         size_t s_slot, size_t s_ws, uint32_t wss)
{
    DecImage im{};
    im.c = img_ptr(containers_, s_slot);
    im.slot_cap = (uint32_t)min(s_slot, (size_t)0xFFFFFFFFu);
    im.valid = valid_bytes_ ? valid_bytes_ + (size_t)blockIdx.y * valid_stride : nullptr;
    im.n = n; im.ns = ns; im.wss = wss;
    im.lat_w = lat_w; im.lat_h = lat_h; im.lat_c = lat_c;
    im.err = const_cast<uint32_t *>(img_ptr(serr_, s_ws));
    im.sums = const_cast<unsigned long long *>(img_ptr(ssum_, s_ws));
    im.status = status_ + 2 * blockIdx.y;
    dec_finish_self_body(im);
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
    const uint32_t ns = (n + stream_symbols(mode) - 1) / stream_symbols(mode);
    if (mode == SICN_CODEC_RANSW) return SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)ns + 2 * (size_t)n + 256 * (size_t)ns;
    if (mode == SICN_CODEC_RAW8) return SICN_CODEC_HEADER_BYTES + (size_t)n;
    if (mode == SICN_CODEC_PACKED7) return SICN_CODEC_HEADER_BYTES + ((size_t)n + 7) / 8 * 7;
    if (mode == SICN_CODEC_RANS) return SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)ns + 2 * (size_t)n + 8 * (size_t)ns;
    return 0;
}

extern "C" size_t sicn_codec_workspace_bytes(int mode, uint32_t n)
{
    Workspace w;
    if (mode == SICN_CODEC_RANSW) {   // enough for a container of ANY admissible stream length (sicn_codec_decode reads it from the header)
        size_t mx = 0;
        for (uint32_t wss = 1024; wss <= WSS; wss <<= 1)
            if (wstream_fits(n, wss)) mx = std::max(mx, carve(w, nullptr, (n + wss - 1) / wss, wstream_cap(wss)) + 64);
        return mx;
    }
    const uint32_t ns = (n + stream_symbols(mode) - 1) / stream_symbols(mode);
    return carve(w, nullptr, ns, mode >= SICN_CODEC_RANS ? stream_cap(mode) : 0) + 64;
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
    if (info->mode == SICN_CODEC_RANSW ? !wstream_ok(info->stream_symbols)
                                       : info->stream_symbols != stream_symbols(info->mode == 4 ? 3 : (int)info->mode))
        return SICN_EINVAL;
    if ((unsigned long long)info->lat_w * info->lat_h * info->lat_c != info->n_symbols) return SICN_EINVAL;
    const uint32_t ss = info->stream_symbols;
    if (info->mode == 4) {   // anchors and non-anchors are cut into streams separately (sicn_codec_ctx.inc)
        const uint32_t W = info->lat_w, H = info->lat_h, C = info->lat_c;
        const unsigned long long na = ((unsigned long long)(H / 2) * W + ((H & 1) ? (W + 1) / 2 : 0)) * C;
        const unsigned long long nn = ((unsigned long long)(H / 2) * W + ((H & 1) ? W / 2 : 0)) * C;
        if (info->n_streams != (na + WSS - 1) / WSS + (nn + WSS - 1) / WSS) return SICN_EINVAL;
        return SICN_OK;
    }
    if (info->n_streams != (info->n_symbols + ss - 1) / ss) return SICN_EINVAL;
    return SICN_OK;
}

extern "C" int sicn_codec_encode(int mode, const uint8_t *latent, uint32_t lat_w, uint32_t lat_h, uint32_t lat_c,
                                 uint32_t img_w, uint32_t img_h, uint8_t *out, size_t out_capacity, size_t *out_bytes,
                                 void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!out || !out_bytes || mode < 0 || mode > 3) return SICN_EINVAL;
    const unsigned long long n64 = (unsigned long long)lat_w * lat_h * lat_c;
    if (n64 > 0x7fffffffull || (n64 && !latent)) return SICN_EINVAL;
    if (mode >= SICN_CODEC_RANS && n64 > MAX_RANS_SYMBOLS) return SICN_EINVAL;
    const uint32_t n = (uint32_t)n64, ss = stream_symbols(mode), ns = (n + ss - 1) / ss;
    if (out_capacity < sicn_codec_max_bytes(mode, n)) return SICN_ENOSPC;
    if (!workspace || workspace_bytes < sicn_codec_workspace_bytes(mode, n)) return SICN_ENOSPC;
    hipStream_t stream = (hipStream_t)hip_stream;
    Workspace w;
    carve(w, workspace, ns, mode >= SICN_CODEC_RANS ? stream_cap(mode) : 0);

    // statistics (also the checksum and the symbol-range check) -------------------------------
    HIP_TRY(hipMemsetAsync(w.hist, 0, 1024 + 64, stream));
    if (n)
        hipLaunchKernelGGL(k_stats, dim3(stats_blocks(n, 1)), dim3(256), 0, stream, latent, n, w.hist, w.sums, (size_t)0, (size_t)0);
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
    put32(head + 36, ss);
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
        if (ns && mode == SICN_CODEC_RANSW)
            hipLaunchKernelGGL(k_ransw_encode, dim3(ns), dim3(64), 0, stream, latent, n, ns, w.freq, w.scratch, w.lens, (size_t)0, (size_t)0, WSS);
        else if (ns)
            hipLaunchKernelGGL(k_rans_encode, dim3((ns + 255) / 256), dim3(256), 0, stream, latent, n, ns, w.freq, w.scratch, w.lens);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, w.lens, (const uint8_t *)nullptr, ns, w.offsets, table, out + 40, (size_t)0, (size_t)0,
                           0xFFFFFFFFu, (uint32_t *)nullptr);
        if (ns) hipLaunchKernelGGL(k_compact, dim3(ns), dim3(256), 0, stream, w.scratch, w.lens, w.offsets, payload, stream_cap(mode), (size_t)0, (size_t)0);
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
    const bool wmode = info.mode == SICN_CODEC_RANSW;
    if (wmode && !wstream_fits(n, info.stream_symbols)) return SICN_EINVAL;
    // (a caller that sized the workspace for the default stream length needs sicn_codec_workspace_bytes_sl for shorter streams)
    if (!workspace || workspace_bytes < (wmode ? sicn_codec_workspace_bytes_sl(n, info.stream_symbols)
                                               : sicn_codec_workspace_bytes((int)info.mode, n)))
        return SICN_ENOSPC;
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
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, (const uint32_t *)nullptr, table, ns, w.offsets,
                           (uint8_t *)nullptr, (uint8_t *)nullptr, (size_t)0, (size_t)0,
                           wmode ? wstream_cap(info.stream_symbols) : stream_cap((int)info.mode), err);
        uint32_t total = 0;
        HIP_TRY(hipMemcpyAsync(&total, w.offsets + ns, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (total != info.payload_bytes) return SICN_EINVAL;
        if (ns && info.mode == SICN_CODEC_RANSW)
            hipLaunchKernelGGL(k_ransw_decode<false>, dim3(ns), dim3(64), 0, stream, payload, freq_bytes, w.offsets, n, ns, latent, err, (size_t)0, (size_t)0, (size_t)0,
                               container + 40, (const uint32_t *)nullptr, (unsigned long long *)nullptr, info.stream_symbols);
        else if (ns)
            hipLaunchKernelGGL(k_rans_decode, dim3((ns + 255) / 256), dim3(256), 0, stream, payload, freq_bytes, w.offsets, n, ns, latent, err,
                               info.payload_bytes);
    }
    // checksum of what was decoded
    uint32_t flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, err, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (flag) return SICN_EINVAL;
    HIP_TRY(hipMemsetAsync(w.hist, 0, 1024 + 64, stream));
    if (n) hipLaunchKernelGGL(k_stats, dim3(stats_blocks(n, 1)), dim3(256), 0, stream, latent, n, w.hist, w.sums, (size_t)0, (size_t)0);
    unsigned long long sums[2];
    HIP_TRY(hipMemcpyAsync(sums, w.sums, sizeof sums, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (hipGetLastError() != hipSuccess) return SICN_ENODEV;
    return adler_from_sums(sums[0], sums[1], n) == info.adler32 ? SICN_OK : SICN_EBADMSG;
}


// ---- batches -------------------------------------------------------------------------------------------------
// The asynchronous pair does everything on the device (statistics -> frequency table -> header -> streams -> offsets
// -> compaction; parse -> offsets -> streams -> checksum) and reports through a device status array: no host
// synchronisation, no allocation, capturable in a hipGraph.  The synchronous batch calls are thin wrappers that add
// the read-back.
extern "C" size_t sicn_codec_batch_workspace_bytes(int mode, uint32_t n_symbols, uint32_t n_images)
{
    // per-image blocks, then room for the synchronous wrappers' status arrays (2 x 8 bytes per image)
    return (size_t)n_images * align_up(sicn_codec_workspace_bytes(mode, n_symbols), 256) + align_up(16 * (size_t)n_images, 256);
}

extern "C" int sicn_codec_encode_batch_async_sl(const uint8_t *latents, uint32_t n_images, uint32_t lat_w, uint32_t lat_h,
                                                uint32_t lat_c, uint32_t img_w, uint32_t img_h, uint8_t *out, size_t slot_bytes,
                                                sicn_codec_status *status_dev, void *workspace, size_t workspace_bytes,
                                                void *hip_stream, uint32_t wss)
{
    if (!out || !status_dev || !wstream_ok(wss)) return SICN_EINVAL;
    const unsigned long long n64 = (unsigned long long)lat_w * lat_h * lat_c;
    if (!wstream_fits(n64, wss) || (n64 && !latents) || n_images > 65535) return SICN_EINVAL;
    if (n_images == 0) return SICN_OK;
    const uint32_t n = (uint32_t)n64, ns = (n + wss - 1) / wss, wcap = wstream_cap(wss);
    if (slot_bytes < sicn_codec_max_bytes_sl(n, wss) || (slot_bytes & 1)) return SICN_ENOSPC;
    const size_t ws1 = align_up(sicn_codec_workspace_bytes_sl(n, wss), 256);
    if (!workspace || workspace_bytes < ws1 * n_images) return SICN_ENOSPC;
    hipStream_t stream = (hipStream_t)hip_stream;
    Workspace w;
    carve(w, workspace, ns, wcap);
    uint32_t *status = (uint32_t *)status_dev;
    uint8_t *table = out + SICN_CODEC_HEADER_BYTES + 256, *payload = table + 4 * (size_t)ns;
    const uint32_t fixed = (uint32_t)(SICN_CODEC_HEADER_BYTES + 256 + 4 * (size_t)ns);
    if (ns && ns <= SELF_SCAN_MAX) {
        // three launches (round 4; four in round 3, six in round 2): statistics in rows (no clear, no atomics) -> streams, every
        // wave making the frequency table from the rows itself and stream 0's wave writing header, table and status ->
        // compaction with its own scan
        const uint32_t n_rows = std::min(std::max(n / 16384u, 1u), STAT_ROWS);
        hipLaunchKernelGGL(k_stats, dim3(n_rows, n_images), dim3(256), 0, stream, latents, n, w.hist, w.sums, (size_t)n, ws1, w.rows);
        const EncSelfHeader sh{w.rows, n_rows, out, slot_bytes, status, lat_w, lat_h, lat_c, img_w, img_h};
        hipLaunchKernelGGL(k_ransw_encode, dim3(ns, n_images), dim3(64), 0, stream, latents, n, ns, w.freq, w.scratch, w.lens,
                           (size_t)n, ws1, wss, sh);
        hipLaunchKernelGGL(k_compact_self, dim3(ns, n_images), dim3(256), 0, stream, w.scratch, w.lens, out, wcap, ns, ws1, slot_bytes,
                           status, fixed);
        return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
    }
    hipLaunchKernelGGL(k_clear_stats, dim3(1, n_images), dim3(64), 0, stream, w.hist, ws1);
    if (n)
        hipLaunchKernelGGL(k_stats, dim3(stats_blocks(n, n_images), n_images), dim3(256), 0, stream, latents, n, w.hist,
                           w.sums, (size_t)n, ws1);
    hipLaunchKernelGGL(k_enc_header, dim3(1, n_images), dim3(64), 0, stream, w.hist, w.sums, w.freq, out, status, n, ns, lat_w,
                       lat_h, lat_c, img_w, img_h, ws1, slot_bytes, wss);
    if (ns)
        hipLaunchKernelGGL(k_ransw_encode, dim3(ns, n_images), dim3(64), 0, stream, latents, n, ns, w.freq, w.scratch, w.lens,
                           (size_t)n, ws1, wss);
    hipLaunchKernelGGL(k_scan, dim3(1, n_images), dim3(1024), 0, stream, w.lens, (const uint8_t *)nullptr, ns, w.offsets, table,
                       out + 40, ws1, slot_bytes, 0xFFFFFFFFu, (uint32_t *)nullptr, status, fixed);
    if (ns)
        hipLaunchKernelGGL(k_compact, dim3(ns, n_images), dim3(256), 0, stream, w.scratch, w.lens, w.offsets, payload, wcap, ws1,
                           slot_bytes);
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
    Workspace w;
    carve(w, workspace, ns, 0);
    const uint8_t *freq_bytes = containers + SICN_CODEC_HEADER_BYTES, *table = freq_bytes + 256, *payload = table + 4 * (size_t)ns;
    if (ns <= SELF_SCAN_MAX) {
        // two launches instead of four: the streams bound and place themselves (self mode), the finish kernel validates header
        // and table and folds the per-stream verdicts / checksum sums (a small image's decode is mostly launch latency)
        uint32_t *serr = w.lens;                                           // [ns]
        unsigned long long *ssum = (unsigned long long *)w.scratch;        // [2 ns]; the scratch slots (>= 2304 B each) are idle in a decode
        const uint32_t *vb = valid_dev_or_null ? &valid_dev_or_null->bytes : (const uint32_t *)nullptr;
        if (ns) {
            // the latency form (one 16 KB table, one LDS round trip less per step) while all waves of the batch fit the chip at
            // five per CU; beyond that the two-table form, whose lookups the other eleven waves of a CU hide
            sicn::ChipGeom chip;
            const bool big = sicn::chip_geom(&chip) == SICN_OK && (unsigned long long)ns * n_images <= 5ull * (unsigned)chip.n_cu;
            if (big)
                hipLaunchKernelGGL(k_ransw_decode<true>, dim3(ns, n_images), dim3(64), 0, stream, payload, freq_bytes, (const uint32_t *)nullptr, n, ns,
                                   latents, serr, slot_bytes, ws1, latent_stride, containers + 40, (const uint32_t *)nullptr, ssum, wss, vb, 2u, 1);
            else
                hipLaunchKernelGGL(k_ransw_decode<false>, dim3(ns, n_images), dim3(64), 0, stream, payload, freq_bytes, (const uint32_t *)nullptr, n, ns,
                                   latents, serr, slot_bytes, ws1, latent_stride, containers + 40, (const uint32_t *)nullptr, ssum, wss, vb, 2u, 1);
        }
        hipLaunchKernelGGL(k_dec_finish_self, dim3(1, n_images), dim3(256), 0, stream, containers, vb, 2u, serr, ssum, (uint32_t *)status_dev,
                           n, ns, lat_w, lat_h, lat_c, slot_bytes, ws1, wss);
        return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
    }
    hipLaunchKernelGGL(k_dec_parse, dim3(1, n_images), dim3(64), 0, stream, containers,
                       valid_dev_or_null ? &valid_dev_or_null->bytes : (const uint32_t *)nullptr, 2u, w.meta, n, ns, lat_w, lat_h,
                       lat_c, slot_bytes, ws1, wss);
    // a slot the parse stage rejected as too short is never read: its table counts as empty (ns_eff = 0 via meta[1] = 0 and
    // the per-stream bound off + len <= payload bytes, so every stream of it flags an error and returns)
    hipLaunchKernelGGL(k_scan, dim3(1, n_images), dim3(1024), 0, stream, (const uint32_t *)nullptr, table, ns, w.offsets,
                       (uint8_t *)nullptr, (uint8_t *)nullptr, ws1, slot_bytes, wstream_cap(wss), w.meta + 3, (uint32_t *)nullptr, 0u,
                       (const uint32_t *)w.meta);
    if (ns)
        hipLaunchKernelGGL(k_ransw_decode<false>, dim3(ns, n_images), dim3(64), 0, stream, payload, freq_bytes, w.offsets, n, ns, latents,
                           w.meta + 3, slot_bytes, ws1, latent_stride, containers + 40, w.meta, w.sums, wss);
    hipLaunchKernelGGL(k_dec_finish, dim3(1, n_images), dim3(64), 0, stream, w.meta, w.hist, w.sums, w.offsets, (uint32_t *)status_dev,
                       n, ns, ws1);
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

static int status_to_rc(uint32_t err)
{
    if (!err) return SICN_OK;
    return (err & ~128u) ? SICN_EINVAL : SICN_EBADMSG;
}

extern "C" int sicn_codec_encode_batch(int mode, const uint8_t *latents, uint32_t n_images, uint32_t lat_w, uint32_t lat_h,
                                       uint32_t lat_c, uint32_t img_w, uint32_t img_h, uint8_t *out, size_t slot_bytes,
                                       size_t *out_bytes_host, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (mode != SICN_CODEC_RANSW || !out || !out_bytes_host) return SICN_EINVAL;
    if (n_images == 0) return SICN_OK;
    // the status array lives behind the per-image blocks of the caller's workspace (sicn_codec_batch_workspace_bytes)
    const unsigned long long n64 = (unsigned long long)lat_w * lat_h * lat_c;
    if (n64 > MAX_RANS_SYMBOLS) return SICN_EINVAL;
    const size_t blocks = (size_t)n_images * align_up(sicn_codec_workspace_bytes(mode, (uint32_t)n64), 256);
    if (!workspace || workspace_bytes < sicn_codec_batch_workspace_bytes(mode, (uint32_t)n64, n_images)) return SICN_ENOSPC;
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

extern "C" int sicn_codec_decode_batch(const uint8_t *containers, size_t slot_bytes, const size_t *bytes_host, uint32_t n_images,
                                       uint8_t *latents, size_t latent_stride, sicn_codec_info *infos_or_null, void *workspace,
                                       size_t workspace_bytes, void *hip_stream)
{
    if (!containers || !bytes_host || (slot_bytes & 1)) return SICN_EINVAL;
    if (n_images == 0) return SICN_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    std::vector<uint8_t> head;
    std::vector<sicn_codec_info> info;
    std::vector<sicn_codec_status> st;
    try {
        head.resize((size_t)n_images * SICN_CODEC_HEADER_BYTES);
        info.resize(n_images);
        st.resize(2 * (size_t)n_images);
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
        st[i].error = 0;
        st[i].bytes = (uint32_t)bytes_host[i];
    }
    const uint32_t wss = info[0].stream_symbols;
    const size_t blocks = (size_t)n_images * align_up(sicn_codec_workspace_bytes_sl(info[0].n_symbols, wss), 256);
    if (!workspace || workspace_bytes < sicn_codec_batch_workspace_bytes_sl(info[0].n_symbols, n_images, wss)) return SICN_ENOSPC;
    sicn_codec_status *st_dev = (sicn_codec_status *)((uint8_t *)workspace + blocks);   // [0, n): valid bytes in, [n, 2n): verdicts out
    int rc = hipMemcpyAsync(st_dev, st.data(), sizeof(sicn_codec_status) * n_images, hipMemcpyHostToDevice, stream) == hipSuccess
                 ? SICN_OK : SICN_ENODEV;
    if (rc == SICN_OK)
        rc = sicn_codec_decode_batch_async_sl(containers, slot_bytes, st_dev, n_images, info[0].lat_w, info[0].lat_h, info[0].lat_c,
                                              latents, latent_stride, st_dev + n_images, workspace, workspace_bytes, hip_stream, wss);
    if (rc == SICN_OK && hipMemcpyAsync(st.data() + n_images, st_dev + n_images, sizeof(sicn_codec_status) * n_images,
                                        hipMemcpyDeviceToHost, stream) != hipSuccess)
        rc = SICN_ENODEV;
    if (hipStreamSynchronize(stream) != hipSuccess) return SICN_ENODEV;
    if (rc) return rc;
    for (uint32_t i = 0; i < n_images; i++)
        if (int e = status_to_rc(st[n_images + i].error)) return e;
    return SICN_OK;
}

#include "sicn_codec_ctx.inc"   // container mode 4: class-conditional rANS-W with a checkerboard context model
