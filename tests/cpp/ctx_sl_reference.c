/*
 * TEST INFRASTRUCTURE — a plain-C statement of container mode 4 ("rANS-WC") with the STREAM LENGTH S as a parameter (header dword 9,
 * a power of two in 1024 .. 16384), written from the format's description in include/sicn_codec.h and oracle/sicn_hyper_oracle.c.
 * The oracle keeps its fixed 16384; tests/test_ctx_stream_length.py holds this file to it where it can speak (S = 16384 byte for
 * byte; a latent whose sets fit one stream at S = 1024, where only dword 9 differs) and to itself elsewhere (round trip, tables
 * independent of S).  Built into a temporary directory by the test module together with oracle/sicn_codec_oracle.c, whose table
 * normalisation and Adler-32 it calls.
 *
 * Format.  Symbols of the latent [H][W][C] (< 128) in two sets, anchors ((x + y) even) then non-anchors, each in raster order over
 * row pairs, channels fastest.  The class of a symbol: anchors scale >> 3; non-anchors min(15, ((scale >> 3) + (m >> 3) + 1) >> 1),
 * m = max of the in-range 4-neighbours (anchors) in the same channel.  16 tables of 128 x u16 (12-bit, per class, from the class
 * histogram; a class without symbols is all zero).  Each set is cut into streams of S symbols, every stream 64 interleaved rANS
 * states over 16-bit words (lane l owns symbols 256 q + 4 l + 0..3), ending with the 64 final states.
 * Container: 48-byte header | 4096 table bytes | u32 length per stream | the streams.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

int sicl_or_normalize(const uint32_t h[128], uint32_t n, uint16_t f[128]);   /* oracle/sicn_codec_oracle.c */
uint32_t sicl_or_adler32(const uint8_t *d, size_t n);

enum { HEADER = 48, CLASSES = 16, TABLES = CLASSES * 256, LANES = 64, PROB = 12 };
#define STATE_LOW (1u << 16)

/* the decoder's verdict classes, named after the status bits of sicn_codec.h */
enum { V_HEADER = 4, V_TABLES = 8, V_PAYLOAD = 16, V_STREAM = 32, V_SUM = 64, V_CHECKSUM = 128, V_SHORT = 0x104 };

static void w32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static uint32_t r32(const uint8_t *p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint32_t r16(const uint8_t *p) { return p[0] | ((uint32_t)p[1] << 8); }

int ctxsl_length_ok(uint32_t S) { return S >= 1024 && S <= 16384 && (S & (S - 1)) == 0; }
uint32_t ctxsl_cap(uint32_t S) { return 2 * S + 256; }      /* one 16-bit word per symbol at most + the 64 final states */

/* symbols of a set: whole row pairs hold W pixels of either set, an odd last row ceil(W/2) anchors and floor(W/2) non-anchors */
uint64_t ctxsl_set_symbols(int set, uint32_t W, uint32_t H, uint32_t C)
{
    const uint64_t last = (H & 1) ? (set == 0 ? (W + 1ull) / 2 : W / 2ull) : 0;
    return ((uint64_t)(H / 2) * W + last) * C;
}
uint64_t ctxsl_set_streams(int set, uint32_t W, uint32_t H, uint32_t C, uint32_t S) { return (ctxsl_set_symbols(set, W, H, C) + S - 1) / S; }
uint64_t ctxsl_streams(uint32_t W, uint32_t H, uint32_t C, uint32_t S) { return ctxsl_set_streams(0, W, H, C, S) + ctxsl_set_streams(1, W, H, C, S); }

/* 0 for a length or a shape outside the limits: W H C <= 0x7F000000, C % 4 == 0, streams * cap(S) < 2^32 */
uint64_t ctxsl_max_bytes(uint32_t W, uint32_t H, uint32_t C, uint32_t S)
{
    if (!ctxsl_length_ok(S) || !W || !H || !C || (C & 3)) return 0;
    const uint64_t n = (uint64_t)W * H * C;
    if ((uint64_t)W * H > 0x7F000000ull || n > 0x7F000000ull) return 0;
    const uint64_t ns = ctxsl_streams(W, H, C, S);
    if (ns * ctxsl_cap(S) >= (1ull << 32)) return 0;
    return HEADER + TABLES + 4 * ns + 2 * n + 256 * ns;
}

/* pixel j of a set -> (y, x) */
static void locate(int set, uint32_t j, uint32_t W, uint32_t *y, uint32_t *x)
{
    const uint32_t half = set == 0 ? (W + 1) / 2 : W / 2, pair = j / W, t = j % W;
    const int upper = t < half;                      /* the pair's even row comes first */
    *y = 2 * pair + (upper ? 0 : 1);
    const uint32_t k = upper ? t : t - half;
    /* in an even row anchors sit at even x, in an odd row at odd x; non-anchors the other way round */
    *x = 2 * k + (((set == 0) == upper) ? 0 : 1);
}

static uint32_t class_of(int set, const uint8_t *lat, const uint8_t *scale, uint32_t W, uint32_t H, uint32_t C, uint32_t y, uint32_t x, uint32_t ch)
{
    const size_t at = ((size_t)y * W + x) * C + ch;
    uint32_t k = scale[at] >> 3;
    if (set == 1) {
        uint32_t m = 0;
        if (y > 0 && lat[at - (size_t)W * C] > m) m = lat[at - (size_t)W * C];
        if (y + 1 < H && lat[at + (size_t)W * C] > m) m = lat[at + (size_t)W * C];
        if (x > 0 && lat[at - C] > m) m = lat[at - C];
        if (x + 1 < W && lat[at + C] > m) m = lat[at + C];
        k = (k + (m >> 3) + 1) >> 1;
    }
    return k > 15 ? 15 : k;
}

static uint32_t owner(uint32_t step, uint32_t lane) { return (step >> 2) * 256u + lane * 4u + (step & 3u); }

/* one stream, written backwards into buf[0 .. cap): returns its length; the stream is buf + cap - length */
static uint32_t put_stream(const uint8_t *sym, const uint8_t *cls, uint32_t n, uint16_t (*freq)[128], uint16_t (*cum)[129], uint8_t *buf,
                           uint32_t cap)
{
    uint32_t state[LANES], at = cap;
    for (int l = 0; l < LANES; l++) state[l] = STATE_LOW;
    for (uint32_t step = (n + 255u) / 256u * 4u; step-- > 0;) {
        for (int l = LANES; l-- > 0;) {               /* renormalise: descending lanes, so that the decoder reads ascending ones */
            const uint32_t j = owner(step, (uint32_t)l);
            if (j >= n) continue;
            const uint32_t f = freq[cls[j]][sym[j]];
            if ((uint64_t)state[l] >= ((uint64_t)f << 20)) {
                at -= 2;
                buf[at] = (uint8_t)state[l];
                buf[at + 1] = (uint8_t)(state[l] >> 8);
                state[l] >>= 16;
            }
        }
        for (int l = 0; l < LANES; l++) {
            const uint32_t j = owner(step, (uint32_t)l);
            if (j >= n) continue;
            const uint32_t f = freq[cls[j]][sym[j]];
            state[l] = ((state[l] / f) << PROB) + state[l] % f + cum[cls[j]][sym[j]];
        }
    }
    for (int l = LANES; l-- > 0;) {
        at -= 4;
        w32(buf + at, state[l]);
    }
    return cap - at;
}

/* Returns the container's bytes, or -22 (a value >= 128, a shape or a length outside the limits), -28 (cap), -12. */
long long ctxsl_encode(const uint8_t *lat, const uint8_t *scale, uint32_t W, uint32_t H, uint32_t C, uint32_t S, uint32_t img_w, uint32_t img_h,
                       uint8_t *out, size_t cap)
{
    const uint64_t need = ctxsl_max_bytes(W, H, C, S);
    if (!need) return -22;
    if (cap < need) return -28;
    const uint32_t n = W * H * C;
    for (uint32_t i = 0; i < n; i++)
        if ((lat[i] | scale[i]) & 0x80) return -22;
    const uint32_t nsym[2] = {(uint32_t)ctxsl_set_symbols(0, W, H, C), (uint32_t)ctxsl_set_symbols(1, W, H, C)};
    const uint32_t nst[2] = {(uint32_t)ctxsl_set_streams(0, W, H, C, S), (uint32_t)ctxsl_set_streams(1, W, H, C, S)};
    uint8_t *sym = (uint8_t *)malloc((size_t)n + 1), *cls = (uint8_t *)malloc((size_t)n + 1), *buf = (uint8_t *)malloc(ctxsl_cap(S));
    if (!sym || !cls || !buf) { free(sym); free(cls); free(buf); return -12; }
    static uint32_t hist[CLASSES][128];
    memset(hist, 0, sizeof hist);
    size_t k = 0;
    for (int set = 0; set < 2; set++)
        for (uint32_t j = 0; j < nsym[set] / C; j++) {
            uint32_t y, x;
            locate(set, j, W, &y, &x);
            for (uint32_t ch = 0; ch < C; ch++, k++) {
                sym[k] = lat[((size_t)y * W + x) * C + ch];
                cls[k] = (uint8_t)class_of(set, lat, scale, W, H, C, y, x, ch);
                hist[cls[k]][sym[k]]++;
            }
        }
    uint16_t freq[CLASSES][128], cum[CLASSES][129];
    for (int c = 0; c < CLASSES; c++) {
        uint32_t total = 0;
        for (int s = 0; s < 128; s++) total += hist[c][s];
        memset(freq[c], 0, sizeof freq[c]);
        if (total && sicl_or_normalize(hist[c], total, freq[c])) { free(sym); free(cls); free(buf); return -22; }
        cum[c][0] = 0;
        for (int s = 0; s < 128; s++) cum[c][s + 1] = (uint16_t)(cum[c][s] + freq[c][s]);
    }
    const uint32_t ns = nst[0] + nst[1];
    const uint32_t head[12] = {0x4C434953u, 1u | (4u << 16), img_w, img_h, W, H, C, n, ns, S, 0, sicl_or_adler32(lat, n)};
    for (int i = 0; i < 12; i++) w32(out + 4 * i, head[i]);
    size_t at = HEADER;
    for (int c = 0; c < CLASSES; c++)
        for (int s = 0; s < 128; s++, at += 2) { out[at] = (uint8_t)freq[c][s]; out[at + 1] = (uint8_t)(freq[c][s] >> 8); }
    uint8_t *lens = out + at;
    at += 4 * (size_t)ns;
    const size_t payload = at;
    size_t base = 0;
    uint32_t st = 0;
    for (int set = 0; set < 2; base += nsym[set], set++)
        for (uint32_t q = 0; q < nst[set]; q++, st++) {
            const uint32_t begin = q * S, left = nsym[set] - begin, cnt = left < S ? left : S;
            const uint32_t len = put_stream(sym + base + begin, cls + base + begin, cnt, freq, cum, buf, ctxsl_cap(S));
            w32(lens + 4 * st, len);
            memcpy(out + at, buf + ctxsl_cap(S) - len, len);
            at += len;
        }
    w32(out + 40, (uint32_t)(at - payload));
    free(sym); free(cls); free(buf);
    return (long long)at;
}

/* The decoder is TOLD the shape and the length it expects, as the library's is.  Returns the symbols decoded, or minus a verdict class
 * (V_*), the first that applies in the order header, tables, payload field, length entries, their sum, streams, checksum.  The latent
 * is zeroed first. */
long long ctxsl_decode(const uint8_t *in, size_t bytes, const uint8_t *scale, uint32_t W, uint32_t H, uint32_t C, uint32_t S, uint8_t *lat)
{
    if (!ctxsl_max_bytes(W, H, C, S)) return -22;
    const uint32_t n = W * H * C;
    const uint32_t nsym[2] = {(uint32_t)ctxsl_set_symbols(0, W, H, C), (uint32_t)ctxsl_set_symbols(1, W, H, C)};
    const uint32_t nst[2] = {(uint32_t)ctxsl_set_streams(0, W, H, C, S), (uint32_t)ctxsl_set_streams(1, W, H, C, S)};
    const uint32_t ns = nst[0] + nst[1];
    memset(lat, 0, n);
    const size_t fixed = HEADER + TABLES + 4 * (size_t)ns;
    if (bytes < fixed) return -V_SHORT;
    const uint32_t expect[10] = {0x4C434953u, 1u | (4u << 16), 0, 0, W, H, C, n, ns, S};
    for (int i = 0; i < 10; i++)
        if (i != 2 && i != 3 && r32(in + 4 * i) != expect[i]) return -V_HEADER;
    uint16_t freq[CLASSES][128], cum[CLASSES][129];
    size_t at = HEADER;
    for (int c = 0; c < CLASSES; c++) {
        uint32_t sum = 0;
        for (int s = 0; s < 128; s++, at += 2) { freq[c][s] = (uint16_t)r16(in + at); sum += freq[c][s]; }
        if (sum != 0 && sum != 4096) return -V_TABLES;
        cum[c][0] = 0;
        for (int s = 0; s < 128; s++) cum[c][s + 1] = (uint16_t)(cum[c][s] + freq[c][s]);
    }
    const uint32_t payload = r32(in + 40);
    if (payload > bytes - fixed) return -V_PAYLOAD;
    const uint8_t *lens = in + at;
    uint64_t total = 0;
    for (uint32_t st = 0; st < ns; st++) {
        if (r32(lens + 4 * st) > ctxsl_cap(S)) return -V_STREAM;      /* no stream of S symbols is longer */
        total += r32(lens + 4 * st);
    }
    if (total != payload) return -V_SUM;
    at = fixed;
    uint32_t st = 0;
    for (int set = 0; set < 2; set++)
        for (uint32_t q = 0; q < nst[set]; q++, st++) {
            const uint32_t len = r32(lens + 4 * st), begin = q * S, left = nsym[set] - begin, cnt = left < S ? left : S;
            if (len < 4 * LANES || (len & 1)) return -V_STREAM;
            const uint8_t *p = in + at, *end = p + len;
            uint32_t state[LANES];
            for (int l = 0; l < LANES; l++, p += 4) state[l] = r32(p);
            for (uint32_t step = 0; step < (cnt + 255u) / 256u * 4u; step++) {
                for (int l = 0; l < LANES; l++) {
                    const uint32_t j = owner(step, (uint32_t)l);
                    if (j >= cnt) continue;
                    const uint32_t e = begin + j, ch = e % C;
                    uint32_t y, x;
                    locate(set, e / C, W, &y, &x);
                    const uint32_t k = class_of(set, lat, scale, W, H, C, y, x, ch), v = state[l] & 4095u;
                    if (cum[k][128] != 4096) return -V_STREAM;       /* a class the container has no table for */
                    uint32_t s = 0;
                    while (cum[k][s + 1] <= v) s++;
                    lat[((size_t)y * W + x) * C + ch] = (uint8_t)s;
                    state[l] = freq[k][s] * (state[l] >> PROB) + v - cum[k][s];
                }
                for (int l = 0; l < LANES; l++) {
                    if (owner(step, (uint32_t)l) >= cnt || state[l] >= STATE_LOW) continue;
                    if (p + 2 > end) return -V_STREAM;
                    state[l] = (state[l] << 16) | r16(p);
                    p += 2;
                }
            }
            for (int l = 0; l < LANES; l++)
                if (state[l] != STATE_LOW) return -V_STREAM;
            if (p != end) return -V_STREAM;
            at += len;
        }
    if (sicl_or_adler32(lat, n) != r32(in + 44)) return -V_CHECKSUM;
    return (long long)n;
}
