// Stand-alone check of csrc/ctx_window_host.hpp (the streams and the band of a window of latent rows of a mode-4 container) for
// builds with the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all ctx_window_plan_check.cpp -o ctx_window_plan_check
// Every output array lives in a heap block of EXACTLY its length, so a write past its end is an AddressSanitizer report, and the
// extreme shapes make an overflowing sum an UndefinedBehaviorSanitizer report, not luck.  The plan is held to brute force over the
// set order (anchors (x + y) even; a set's pixels in raster order, channels fastest).  Exit status 0 and one line
// "ctx_window_plan_check ok: <n> checks" when everything held.  No device, no library.
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

// the set order by brute force: a pixel's C symbols may straddle two streams, so the first and the last stream of every pixel
struct Order {
    uint32_t W, H, C;
    std::vector<uint32_t> first, last;   // [H][W], in the pixel's own set
    std::vector<uint64_t> nsym;
    Order(uint32_t w, uint32_t h, uint32_t c) : W(w), H(h), C(c), first((size_t)w * h), last((size_t)w * h), nsym(2, 0)
    {
        uint64_t at[2] = {0, 0};
        for (uint32_t y = 0; y < H; y++)
            for (uint32_t x = 0; x < W; x++) {
                const int s = (x + y) & 1;
                first[(size_t)y * W + x] = (uint32_t)(at[s] / sicn_ctx_window::WSS);
                last[(size_t)y * W + x] = (uint32_t)((at[s] + C - 1) / sicn_ctx_window::WSS);
                at[s] += C;
            }
        nsym[0] = at[0];
        nsym[1] = at[1];
    }
};

void sufficient(const Order &o, uint32_t r0, uint32_t rh)
{
    auto im = exact<sicn_ragged_ctx_window_image>(1);
    EXPECT(sicn_ctx_window::plan_of(o.W, o.H, o.C, r0, rh, 32, im.get()) == SICN_OK);
    const sicn_ragged_ctx_window_image &p = im[0];
    EXPECT(p.band_offset == 32 && p.band_bytes == (uint64_t)p.band_rows * o.W * o.C);
    EXPECT(p.band_row0 <= r0 && r0 + rh <= p.band_row0 + p.band_rows && p.band_row0 + p.band_rows <= o.H);
    auto in = [&](int s, uint32_t st) { return st >= p.first_stream[s] && st < p.end_stream[s]; };
    uint64_t held = 0;
    for (int s = 0; s < 2; s++) {
        const uint64_t nst = (o.nsym[s] + sicn_ctx_window::WSS - 1) / sicn_ctx_window::WSS;
        EXPECT(p.end_stream[s] <= nst && p.first_stream[s] <= p.end_stream[s]);
        held += std::min<uint64_t>(o.nsym[s], (uint64_t)p.end_stream[s] * sicn_ctx_window::WSS) - (uint64_t)p.first_stream[s] * sicn_ctx_window::WSS;
    }
    EXPECT(held == p.symbols);
    bool ok = true;
    for (uint32_t y = 0; y < o.H && ok; y++)
        for (uint32_t x = 0; x < o.W && ok; x++) {
            const int s = (x + y) & 1;
            const size_t at = (size_t)y * o.W + x;
            const bool some = in(s, o.first[at]) || in(s, o.last[at]), all = in(s, o.first[at]) && in(s, o.last[at]);
            if (y >= r0 && y < r0 + rh) ok = ok && all;                                           // the wanted rows are held
            if (some) ok = ok && y >= p.band_row0 && y < p.band_row0 + p.band_rows;               // nothing lands outside the band
            if (s == 1 && some) {                                                                 // every neighbour of a held non-anchor is held
                if (y > 0) ok = ok && in(0, o.first[at - o.W]) && in(0, o.last[at - o.W]);
                if (y + 1 < o.H) ok = ok && in(0, o.first[at + o.W]) && in(0, o.last[at + o.W]);
                if (x > 0) ok = ok && in(0, o.first[at - 1]) && in(0, o.last[at - 1]);
                if (x + 1 < o.W) ok = ok && in(0, o.first[at + 1]) && in(0, o.last[at + 1]);
            }
        }
    EXPECT(ok);
}

void plans()
{
    const uint32_t shapes[][3] = {{1, 1, 4}, {2, 2, 4}, {5, 1, 192}, {1, 5, 192}, {3, 3, 192}, {37, 37, 192}, {48, 40, 192}, {1, 171, 192},
                                  {86, 86, 192}, {201, 37, 192}};   // W, H, C
    for (const auto &s : shapes) {
        const Order o(s[0], s[1], s[2]);
        const uint32_t H = s[1], step = H > 60 ? 5 : 1;
        for (uint32_t r0 = 0; r0 < H; r0 += step)
            for (uint32_t rh = 1; r0 + rh <= H; rh += (H > 60 ? 7 : 1)) sufficient(o, r0, rh);
        sufficient(o, 0, H);
        sufficient(o, H - 1, 1);
        // the whole image selects every stream and the band is the latent
        sicn_ragged_ctx_window_image im;
        EXPECT(sicn_ctx_window::plan_of(s[0], s[1], s[2], 0, H, 0, &im) == SICN_OK);
        EXPECT(im.band_row0 == 0 && im.band_rows == H && im.symbols == (uint64_t)s[0] * s[1] * s[2] && im.first_stream[0] == 0 && im.first_stream[1] == 0);
        EXPECT(im.end_stream[0] == (o.nsym[0] + 16383) / 16384 && im.end_stream[1] == (o.nsym[1] + 16383) / 16384);
    }
}

void limits()
{
    sicn_ragged_ctx_window_image im;
    EXPECT(sicn_ctx_window::plan_of(4, 4, 4, 0, 0, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::plan_of(4, 4, 4, 4, 1, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::plan_of(4, 4, 4, 3, 2, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::plan_of(4, 4, 4, UINT32_MAX, UINT32_MAX, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::plan_of(4, 4, 4, 1, UINT32_MAX, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::plan_of(4, 4, 6, 0, 1, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::plan_of(4, 4, 0, 0, 1, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::plan_of(0, 4, 4, 0, 1, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::plan_of(4, 0, 4, 0, 1, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::plan_of(UINT32_MAX, UINT32_MAX, 0xFFFFFFFCu, 0, 1, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::plan_of(4, 4, 4, 0, 1, 0, nullptr) == SICN_EINVAL);
    // the largest image the coder takes, its last row and all of it: nothing wraps
    const uint32_t W = 0x7F0000u / 4, H = 256, C = 4;                    // W H C = 0x7F000000
    EXPECT(sicn_ctx_window::plan_of(W, H, C, H - 1, 1, 0, &im) == SICN_OK && im.band_row0 + im.band_rows == H && im.band_row0 <= H - 2);
    EXPECT(sicn_ctx_window::plan_of(W, H, C, 0, H, 0, &im) == SICN_OK && im.band_bytes == 0x7F000000u && im.symbols == 0x7F000000u);
    EXPECT(sicn_ctx_window::plan_of(W + 1, H, C, 0, 1, 0, &im) == SICN_EINVAL);

    // a batch: exactly n entries written, offsets 64-bit and multiples of 16
    const int n = 5;
    auto lw = exact<uint32_t>(n), lh = exact<uint32_t>(n), r0 = exact<uint32_t>(n), rh = exact<uint32_t>(n);
    for (int i = 0; i < n; i++) { lw[i] = W; lh[i] = H; r0[i] = 0; rh[i] = H; }
    lw[1] = 3; lh[1] = 3; r0[1] = 1; rh[1] = 1;                          // 3 x 3 x 4: 36 band bytes, rounded up to 48
    auto images = exact<sicn_ragged_ctx_window_image>(n);
    auto streams = exact<uint64_t>(2);
    uint64_t total = 0;
    EXPECT(sicn_ctx_window::window_layout(lw.get(), lh.get(), 4, r0.get(), rh.get(), n, images.get(), &total, streams.get()) == SICN_OK);
    EXPECT(total == 4 * 0x7F000000ull + 48 && images[n - 1].band_offset == 3 * 0x7F000000ull + 48 && images[2].band_offset == 0x7F000000ull + 48);
    EXPECT(streams[0] == 4 * (0x7F000000ull / 2 / 16384) + 1 && streams[1] == streams[0]);
    for (int i = 0; i < n; i++) EXPECT(images[i].band_offset % 16 == 0);
    rh[n - 1] = H + 1;
    EXPECT(sicn_ctx_window::window_layout(lw.get(), lh.get(), 4, r0.get(), rh.get(), n, nullptr, nullptr, nullptr) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::window_layout(lw.get(), lh.get(), 4, r0.get(), rh.get(), 0, nullptr, nullptr, nullptr) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::window_layout(nullptr, lh.get(), 4, r0.get(), rh.get(), 1, nullptr, nullptr, nullptr) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::window_layout(lw.get(), lh.get(), 4, nullptr, rh.get(), 1, nullptr, nullptr, nullptr) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::window_layout(lw.get(), lh.get(), 4, r0.get(), nullptr, 1, nullptr, nullptr, nullptr) == SICN_EINVAL);
    EXPECT(sicn_ctx_window::window_layout(lw.get(), lh.get(), 4, r0.get(), rh.get(), 1, nullptr, nullptr, nullptr) == SICN_OK);
}

}  // namespace

int main()
{
    plans();
    limits();
    std::printf("ctx_window_plan_check ok: %lld checks\n", checks);
    return 0;
}
