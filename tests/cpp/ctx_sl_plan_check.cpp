// Stand-alone check of the host arithmetic of the rANS-WC stream length (include/sicn_ctx_stream_length.h) for builds with the host
// sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all ctx_sl_plan_check.cpp -o ctx_sl_plan_check
// csrc/ctx_window_host.hpp with the stream length S a parameter — the plan of a window held to brute force over the set order at every
// admissible S, into heap blocks of EXACTLY their length, with the extreme shapes and every refusal.  Exit status 0 and one line
// "ctx_sl_plan_check ok: <n> checks" when everything held.  No device, no library.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../simple_image_compression_network_amd/csrc/ctx_window_host.hpp"

namespace {

long long checks = 0;

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        checks++;                                                                     \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

template <class T>
std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }

const uint32_t LENGTHS[] = {1024, 2048, 4096, 8192, 16384};

// where every pixel's C symbols start in its own set (anchors (x + y) even; raster order inside a set, channels fastest)
struct Order {
    uint32_t W, H, C;
    std::vector<uint64_t> at;   // [H][W]
    uint64_t nsym[2] = {0, 0};
    Order(uint32_t w, uint32_t h, uint32_t c) : W(w), H(h), C(c), at((size_t)w * h)
    {
        for (uint32_t y = 0; y < H; y++)
            for (uint32_t x = 0; x < W; x++) {
                const int s = (x + y) & 1;
                at[(size_t)y * W + x] = nsym[s];
                nsym[s] += C;
            }
    }
};

void sufficient(const Order &o, uint32_t S, uint32_t r0, uint32_t rh)
{
    auto im = exact<sicn_ragged_ctx_window_image>(1);
    EXPECT(sicn_ctx_window::plan_of_sl(o.W, o.H, o.C, S, r0, rh, 48, im.get()) == SICN_OK);
    const sicn_ragged_ctx_window_image &p = im[0];
    EXPECT(p.band_offset == 48 && p.band_bytes == (uint64_t)p.band_rows * o.W * o.C);
    EXPECT(p.band_row0 <= r0 && r0 + rh <= p.band_row0 + p.band_rows && p.band_row0 + p.band_rows <= o.H);
    uint64_t held = 0;
    for (int s = 0; s < 2; s++) {
        const uint64_t nst = (o.nsym[s] + S - 1) / S;
        EXPECT(p.end_stream[s] <= nst && p.first_stream[s] <= p.end_stream[s]);
        held += std::min<uint64_t>(o.nsym[s], (uint64_t)p.end_stream[s] * S) - (uint64_t)p.first_stream[s] * S;
    }
    EXPECT(held == p.symbols);
    auto in = [&](int s, uint64_t symbol) { const uint64_t st = symbol / S; return st >= p.first_stream[s] && st < p.end_stream[s]; };
    auto whole = [&](int s, size_t px) { return in(s, o.at[px]) && in(s, o.at[px] + o.C - 1); };
    bool ok = true;
    for (uint32_t y = 0; y < o.H && ok; y++)
        for (uint32_t x = 0; x < o.W && ok; x++) {
            const int s = (x + y) & 1;
            const size_t px = (size_t)y * o.W + x;
            const bool some = in(s, o.at[px]) || in(s, o.at[px] + o.C - 1);
            if (y >= r0 && y < r0 + rh) ok = ok && whole(s, px);                                  // the wanted rows are held
            if (some) ok = ok && y >= p.band_row0 && y < p.band_row0 + p.band_rows;               // nothing lands outside the band
            if (s == 1 && some) {                                                                 // every neighbour of a held non-anchor is held
                if (y > 0) ok = ok && whole(0, px - o.W);
                if (y + 1 < o.H) ok = ok && whole(0, px + o.W);
                if (x > 0) ok = ok && whole(0, px - 1);
                if (x + 1 < o.W) ok = ok && whole(0, px + 1);
            }
        }
    EXPECT(ok);
}

void window_plans()
{
    const uint32_t shapes[][3] = {{1, 1, 4}, {2, 2, 4}, {1, 5, 192}, {5, 1, 192}, {3, 3, 192}, {37, 37, 192}, {48, 40, 192}, {33, 16, 4}, {32, 17, 4}};   // W, H, C
    for (const auto &s : shapes) {
        const Order o(s[0], s[1], s[2]);
        const uint32_t H = s[1];
        for (uint32_t S : LENGTHS) {
            for (uint32_t r0 = 0; r0 < H; r0++)
                for (uint32_t rh = 1; r0 + rh <= H; rh++) sufficient(o, S, r0, rh);
            sicn_ragged_ctx_window_image im;
            EXPECT(sicn_ctx_window::plan_of_sl(s[0], s[1], s[2], S, 0, H, 0, &im) == SICN_OK);
            EXPECT(im.band_row0 == 0 && im.band_rows == H && im.symbols == (uint64_t)s[0] * s[1] * s[2]);
            EXPECT(im.end_stream[0] == (o.nsym[0] + S - 1) / S && im.end_stream[1] == (o.nsym[1] + S - 1) / S);
        }
        // the plan without a length is the plan at 16384, field for field
        sicn_ragged_ctx_window_image a, b;
        const uint32_t r0 = H / 3, rh = H - r0 > 1 ? (H - r0) / 2 : 1;
        EXPECT(sicn_ctx_window::plan_of(s[0], s[1], s[2], r0, rh, 16, &a) == SICN_OK);
        EXPECT(sicn_ctx_window::plan_of_sl(s[0], s[1], s[2], 16384, r0, rh, 16, &b) == SICN_OK);
        EXPECT(a.band_offset == b.band_offset && a.band_bytes == b.band_bytes && a.band_row0 == b.band_row0 && a.band_rows == b.band_rows &&
               a.symbols == b.symbols && a.first_stream[0] == b.first_stream[0] && a.first_stream[1] == b.first_stream[1] &&
               a.end_stream[0] == b.end_stream[0] && a.end_stream[1] == b.end_stream[1]);
    }
    // a band can only shrink with S
    for (uint32_t r0 = 0; r0 < 40; r0 += 3) {
        uint32_t before = 0;
        for (uint32_t S : LENGTHS) {
            sicn_ragged_ctx_window_image im;
            EXPECT(sicn_ctx_window::plan_of_sl(48, 40, 192, S, r0, std::min(40u - r0, 9u), 0, &im) == SICN_OK);
            EXPECT(im.band_rows >= before);
            before = im.band_rows;
        }
    }
}

void refusals_and_limits()
{
    sicn_ragged_ctx_window_image im;
    for (uint32_t bad : {0u, 1u, 512u, 1023u, 1025u, 1536u, 3072u, 16383u, 16385u, 32768u, 0x80000000u, UINT32_MAX})
        EXPECT(sicn_ctx_window::plan_of_sl(4, 4, 4, bad, 0, 1, 0, &im) == SICN_EINVAL);
    for (uint32_t S : LENGTHS) {
        EXPECT(sicn_ctx_window::length_ok(S));
        EXPECT(sicn_ctx_window::plan_of_sl(4, 4, 4, S, 0, 0, 0, &im) == SICN_EINVAL);
        EXPECT(sicn_ctx_window::plan_of_sl(4, 4, 4, S, 3, 2, 0, &im) == SICN_EINVAL);
        EXPECT(sicn_ctx_window::plan_of_sl(4, 4, 4, S, UINT32_MAX, UINT32_MAX, 0, &im) == SICN_EINVAL);
        EXPECT(sicn_ctx_window::plan_of_sl(4, 4, 6, S, 0, 1, 0, &im) == SICN_EINVAL);
        EXPECT(sicn_ctx_window::plan_of_sl(0, 4, 4, S, 0, 1, 0, &im) == SICN_EINVAL);
        EXPECT(sicn_ctx_window::plan_of_sl(4, 4, 4, S, 0, 1, 0, nullptr) == SICN_EINVAL);
        // the largest image: 0x7F000000 symbols (the arithmetic itself has no limit below that; the coder's layout adds the stream limit)
        const uint32_t W = 0x7F0000 / 4, H = 256, C = 4;
        EXPECT(sicn_ctx_window::plan_of_sl(W, H, C, S, H - 1, 1, 0, &im) == SICN_OK && im.band_row0 + im.band_rows == H && im.band_row0 <= H - 2);
        EXPECT(sicn_ctx_window::plan_of_sl(W, H, C, S, 0, H, 0, &im) == SICN_OK && im.band_bytes == 0x7F000000u && im.symbols == 0x7F000000u);
        EXPECT(im.end_stream[0] + im.end_stream[1] == 0x7F000000u / S);
        EXPECT(sicn_ctx_window::plan_of_sl(W + 1, H, C, S, 0, 1, 0, &im) == SICN_EINVAL);
    }
    // a batch with a length per image, outputs of exactly n entries
    const int n = 7;
    auto lw = exact<uint32_t>(n), lh = exact<uint32_t>(n), ss = exact<uint32_t>(n), r0 = exact<uint32_t>(n), rh = exact<uint32_t>(n);
    auto images = exact<sicn_ragged_ctx_window_image>(n);
    auto streams = exact<uint64_t>(2);
    for (int i = 0; i < n; i++) { lw[i] = 37 + (uint32_t)i; lh[i] = 20 + (uint32_t)i; ss[i] = LENGTHS[i % 5]; r0[i] = (uint32_t)i; rh[i] = 5; }
    uint64_t total = 0, at = 0, sel[2] = {0, 0};
    EXPECT(sicn_ctx_window::window_layout_sl(lw.get(), lh.get(), 192, ss.get(), r0.get(), rh.get(), n, images.get(), &total, streams.get()) == SICN_OK);
    for (int i = 0; i < n; i++) {
        sicn_ragged_ctx_window_image one;
        EXPECT(sicn_ctx_window::plan_of_sl(lw[i], lh[i], 192, ss[i], r0[i], rh[i], at, &one) == SICN_OK);
        EXPECT(images[i].band_offset == at && images[i].band_rows == one.band_rows && images[i].symbols == one.symbols);
        at += sicn_ctx_window::a16(one.band_bytes);
        for (int s = 0; s < 2; s++) sel[s] += one.end_stream[s] - one.first_stream[s];
    }
    EXPECT(total == at && streams[0] == sel[0] && streams[1] == sel[1]);
    ss[3] = 1536;
    EXPECT(sicn_ctx_window::window_layout_sl(lw.get(), lh.get(), 192, ss.get(), r0.get(), rh.get(), n, nullptr, nullptr, nullptr) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::window_layout_sl(lw.get(), lh.get(), 192, nullptr, r0.get(), rh.get(), n, nullptr, &total, nullptr) == SICN_OK);
    uint64_t old = 0;
    EXPECT(sicn_ctx_window::window_layout(lw.get(), lh.get(), 192, r0.get(), rh.get(), n, nullptr, &old, nullptr) == SICN_OK && old == total);
}

}  // namespace

int main()
{
    window_plans();
    refusals_and_limits();
    std::printf("ctx_sl_plan_check ok: %lld checks\n", checks);
    return 0;
}
