// Stand-alone check of csrc/window_host.hpp (the ROI plan, the band of a window of latent rows, the tables of the cut) for builds
// with the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all window_plan_check.cpp -o window_plan_check
// Every output array lives in a heap block of EXACTLY its length, so a write past its end is an AddressSanitizer report, and the
// extreme coordinates make an overflowing sum an UndefinedBehaviorSanitizer report, not luck.  Exit status 0 and one line
// "window_plan_check ok: <n> checks" when everything held.  No device, no library.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../simple_image_compression_network_amd/csrc/window_host.hpp"

namespace {

int checks = 0;

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

// the closed form once more, one axis
void window(int64_t p0, int64_t len, int64_t lat, int64_t lo, int64_t hi, int64_t scale, int64_t *first, int64_t *count)
{
    int64_t a = p0 - lo >= 0 ? (p0 - lo) / scale : 0;
    int64_t b = (p0 + len + hi + scale - 1) / scale;
    if (b > lat) b = lat;
    *first = a;
    *count = b - a;
}

void plans()
{
    // every rectangle of a 50 x 37 image (latent 4 x 3) with a few sizes: the plan is the closed form
    const int W = 50, H = 37, LW = 4, LH = 3;
    for (int x0 = 0; x0 < W; x0++)
        for (int y0 = 0; y0 < H; y0 += 3)
            for (int w : {1, 2, 17, W - x0})
                for (int h : {1, 16, H - y0}) {
                    const sicn_ragged_rect r{x0, y0, w, h};
                    auto out = exact<sicn_ragged_roi>(1);
                    const int rc = sicn_window::roi_plan(4, W, H, LW, LH, &r, out.get());
                    if (w > W - x0 || h > H - y0) {
                        EXPECT(rc == SICN_EINVAL);
                        continue;
                    }
                    EXPECT(rc == SICN_OK);
                    int64_t c0, cw, r0, rh;
                    window(x0, w, LW, 15, 30, 16, &c0, &cw);
                    window(y0, h, LH, 15, 30, 16, &r0, &rh);
                    EXPECT(out[0].c0 == c0 && out[0].cw == cw && out[0].r0 == r0 && out[0].rh == rh);
                    EXPECT(out[0].x == x0 - 16 * c0 && out[0].y == y0 - 16 * r0);
                    EXPECT(out[0].cw >= 1 && out[0].rh >= 1 && out[0].x + w <= 16 * out[0].cw && out[0].y + h <= 16 * out[0].rh);
                }
    // margins for every admissible layer count, and the largest sizes
    for (int l = 1; l <= sicn_window::MAX_UP_LAYERS; l++) {
        int64_t lo = 0, hi = 0;
        for (int k = 0; k < l; k++) { lo = 2 * lo + 1; hi = 2 * hi + 2; }      // m' = 2 m + 1, n' = 2 n + 2 per deconv522 layer
        EXPECT(lo == sicn_window::margin_lo(l) && hi == sicn_window::margin_hi(l));
        EXPECT(lo == ((int64_t)1 << l) - 1 && hi == 2 * (((int64_t)1 << l) - 1));
    }
    sicn_ragged_roi out;
    const int32_t big = 1 << 20;
    sicn_ragged_rect r{16 * big - 1, 16 * big - 1, 1, 1};
    EXPECT(sicn_window::roi_plan(4, 16 * big, 16 * big, big, big, &r, &out) == SICN_OK && out.c0 + out.cw == big && out.x == 15);
    r = sicn_ragged_rect{INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    EXPECT(sicn_window::roi_plan(4, 16 * big, 16 * big, big, big, &r, &out) == SICN_EINVAL);
    r = sicn_ragged_rect{INT_MIN, INT_MIN, INT_MAX, INT_MAX};
    EXPECT(sicn_window::roi_plan(4, INT_MAX, INT_MAX, big, big, &r, &out) == SICN_EINVAL);
    r = sicn_ragged_rect{0, 0, INT_MIN, 1};
    EXPECT(sicn_window::roi_plan(4, 16, 16, 1, 1, &r, &out) == SICN_EINVAL);
    r = sicn_ragged_rect{0, 0, 1, 1};
    EXPECT(sicn_window::roi_plan(12, INT_MAX, INT_MAX, big, big, &r, &out) == SICN_OK);
    EXPECT(sicn_window::roi_plan(4, 16, 16, INT_MAX, 1, &r, &out) == SICN_EINVAL);
    EXPECT(sicn_window::roi_plan(0, 16, 16, 1, 1, &r, &out) == SICN_EINVAL);
    EXPECT(sicn_window::roi_plan(13, 16, 16, 1, 1, &r, &out) == SICN_EINVAL);
    EXPECT(sicn_window::roi_plan(4, 16, 16, 1, 1, nullptr, &out) == SICN_EINVAL);
    EXPECT(sicn_window::roi_plan(4, 16, 16, 1, 1, &r, nullptr) == SICN_EINVAL);
}

void bands()
{
    // every window of rows of a few shapes at every stream length: the band holds the rows and nothing of another stream range
    const uint32_t shapes[][3] = {{7, 9, 192}, {16, 3, 192}, {1, 1, 192}, {13, 11, 5}, {120, 68, 192}};
    for (const auto &s : shapes)
        for (uint32_t wss = 1024; wss <= 16384; wss *= 2)
            for (uint32_t r0 = 0; r0 < s[1]; r0 += (s[1] > 20 ? 7 : 1))
                for (uint32_t rh = 1; r0 + rh <= s[1]; rh += (s[1] > 20 ? 11 : 1)) {
                    auto im = exact<sicn_ragged_window_image>(1);
                    EXPECT(sicn_window::band_of(s[0], s[1], s[2], wss, r0, rh, 48, im.get()) == SICN_OK);
                    const uint64_t n = (uint64_t)s[0] * s[1] * s[2], row = (uint64_t)s[0] * s[2];
                    EXPECT((uint64_t)im[0].first_stream * wss <= r0 * row && r0 * row < ((uint64_t)im[0].first_stream + 1) * wss);
                    EXPECT((uint64_t)im[0].end_stream * wss >= (r0 + rh) * row && ((uint64_t)im[0].end_stream - 1) * wss < (r0 + rh) * row);
                    EXPECT(im[0].lead == r0 * row - (uint64_t)im[0].first_stream * wss);
                    EXPECT(im[0].lead + rh * row <= im[0].band_bytes);
                    EXPECT((uint64_t)im[0].first_stream * wss + im[0].band_bytes <= n && im[0].band_offset == 48);
                }
    sicn_ragged_window_image im;
    EXPECT(sicn_window::band_of(4, 4, 4, 1024, 0, 0, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_window::band_of(4, 4, 4, 1024, 4, 1, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_window::band_of(4, 4, 4, 1024, 3, 2, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_window::band_of(4, 4, 4, 1024, UINT32_MAX, UINT32_MAX, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_window::band_of(4, 4, 4, 1024, 1, UINT32_MAX, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_window::band_of(UINT32_MAX, UINT32_MAX, UINT32_MAX, 16384, 0, 1, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_window::band_of(4, 4, 4, 1000, 0, 1, 0, &im) == SICN_EINVAL);
    EXPECT(sicn_window::band_of(4096, 8192, 1, 16384, 8191, 1, 0, &im) == SICN_OK && im.end_stream == 2048);

    // a batch: exactly n entries written, offsets 64-bit and multiples of 16
    const int n = 150;
    auto lw = exact<uint32_t>(n), lh = exact<uint32_t>(n), r0 = exact<uint32_t>(n), rh = exact<uint32_t>(n);
    for (int i = 0; i < n; i++) { lw[i] = 4096; lh[i] = 8192; r0[i] = 0; rh[i] = 8192; }
    auto images = exact<sicn_ragged_window_image>(n);
    uint64_t total = 0, streams = 0;
    EXPECT(sicn_window::window_layout(lw.get(), lh.get(), 1, nullptr, r0.get(), rh.get(), n, images.get(), &total, &streams) == SICN_OK);
    EXPECT(total == (uint64_t)n << 25 && streams == (uint64_t)n * 2048 && images[n - 1].band_offset == (uint64_t)(n - 1) << 25);
    rh[n - 1] = 8193;
    EXPECT(sicn_window::window_layout(lw.get(), lh.get(), 1, nullptr, r0.get(), rh.get(), n, nullptr, nullptr, nullptr) == SICN_EINVAL);
    EXPECT(sicn_window::window_layout(lw.get(), lh.get(), 1, nullptr, r0.get(), rh.get(), 0, nullptr, nullptr, nullptr) == SICN_EINVAL);
    EXPECT(sicn_window::window_layout(nullptr, lh.get(), 1, nullptr, r0.get(), rh.get(), 1, nullptr, nullptr, nullptr) == SICN_EINVAL);
}

void cuts()
{
    const int n = 5;
    auto sw = exact<int32_t>(n), sh = exact<int32_t>(n);
    auto rects = exact<sicn_ragged_rect>(n);
    const int32_t src[n][2] = {{7, 9}, {16, 3}, {1, 1}, {100, 131}, {1 << 20, 1}};
    const sicn_ragged_rect rr[n] = {{2, 3, 4, 5}, {0, 0, 16, 3}, {0, 0, 1, 1}, {99, 130, 1, 1}, {(1 << 20) - 1, 0, 1, 1}};
    for (int i = 0; i < n; i++) { sw[i] = src[i][0]; sh[i] = src[i][1]; rects[i] = rr[i]; }
    for (int channels : {3, 16, 192, 193}) {
        auto rows = exact<sicn_window::CutRow>(n);
        auto first = exact<int64_t>(n + 1), off = exact<int64_t>(n);
        int64_t totals[2];
        EXPECT(sicn_window::cut_plan(sw.get(), sh.get(), rects.get(), channels, nullptr, n, rows.get(), first.get(), off.get(), totals) == SICN_OK);
        int64_t so = 0, dof = 0, item = 0;
        for (int i = 0; i < n; i++) {
            const int64_t srow = (int64_t)sw[i] * channels, drow = (int64_t)rects[i].w * channels;
            EXPECT(off[i] == so && first[i] == item && rows[i].first_item == item && rows[i].dst_off == dof);
            EXPECT(rows[i].src_off == so + rects[i].y0 * srow + (int64_t)rects[i].x0 * channels);
            EXPECT(rows[i].src_row == srow && rows[i].dst_row == drow && rows[i].dst_h == (uint32_t)rects[i].h);
            EXPECT(rows[i].vec == (uint32_t)(((srow | drow | rows[i].src_off | dof) & 15) == 0));
            // the last byte the kernel reads lies inside the source image
            EXPECT(rows[i].src_off + (rects[i].h - 1) * srow + drow <= so + srow * sh[i]);
            so += srow * sh[i];
            dof += drow * rects[i].h;
            item += (rects[i].h + sicn_window::CUT_ROWS - 1) / sicn_window::CUT_ROWS;
        }
        EXPECT(first[n] == item && totals[0] == so && totals[1] == dof);
        // explicit offsets
        auto offs = exact<uint64_t>(n);
        for (int i = 0; i < n; i++) offs[i] = 6000000000ull - 1000000ull * i * i + (channels == 16 ? 16 : 3);
        EXPECT(sicn_window::cut_plan(sw.get(), sh.get(), rects.get(), channels, offs.get(), n, rows.get(), nullptr, off.get(), totals) == SICN_OK);
        for (int i = 0; i < n; i++) EXPECT(off[i] == (int64_t)offs[i] && rows[i].src_off >= off[i]);
        int64_t reach = 0;
        for (int i = 0; i < n; i++) reach = std::max(reach, (int64_t)offs[i] + (int64_t)sw[i] * sh[i] * channels);
        EXPECT(totals[0] == reach);
    }
    int64_t totals[2];
    const int32_t w8 = 8, big = 1 << 16, half = 1 << 15, over = (1 << 20) + 1, zero = 0;
    sicn_ragged_rect r{1, 1, 4, 4};
    EXPECT(sicn_window::cut_plan(&w8, &w8, &r, 3, nullptr, 1, nullptr, nullptr, nullptr, totals) == SICN_OK && totals[1] == 48);
    for (const sicn_ragged_rect &bad : {sicn_ragged_rect{1, 1, 0, 4}, {1, 1, 4, 0}, {-1, 1, 4, 4}, {1, -1, 4, 4}, {5, 1, 4, 4}, {1, 5, 4, 4},
                                        {INT_MAX, 0, INT_MAX, 1}, {0, INT_MAX, 1, INT_MAX}, {INT_MIN, INT_MIN, INT_MAX, INT_MAX},
                                        {0, 0, INT_MIN, INT_MIN}})
        EXPECT(sicn_window::cut_plan(&w8, &w8, &bad, 3, nullptr, 1, nullptr, nullptr, nullptr, totals) == SICN_EINVAL);
    EXPECT(sicn_window::cut_plan(&w8, &w8, &r, 0, nullptr, 1, nullptr, nullptr, nullptr, totals) == SICN_EINVAL);
    EXPECT(sicn_window::cut_plan(&w8, &w8, &r, 3, nullptr, 0, nullptr, nullptr, nullptr, totals) == SICN_EINVAL);
    EXPECT(sicn_window::cut_plan(&zero, &w8, &r, 3, nullptr, 1, nullptr, nullptr, nullptr, totals) == SICN_EINVAL);
    EXPECT(sicn_window::cut_plan(&w8, &over, &r, 3, nullptr, 1, nullptr, nullptr, nullptr, totals) == SICN_EINVAL);
    EXPECT(sicn_window::cut_plan(&big, &half, &r, 1, nullptr, 1, nullptr, nullptr, nullptr, totals) == SICN_EINVAL);
    EXPECT(sicn_window::cut_plan(&big, &half, &r, INT_MAX, nullptr, 1, nullptr, nullptr, nullptr, totals) == SICN_EINVAL);
    const uint64_t far = (uint64_t)1 << 62, near = far - 1;
    EXPECT(sicn_window::cut_plan(&w8, &w8, &r, 3, &far, 1, nullptr, nullptr, nullptr, totals) == SICN_EINVAL);
    EXPECT(sicn_window::cut_plan(&w8, &w8, &r, 3, &near, 1, nullptr, nullptr, nullptr, totals) == SICN_OK);
    EXPECT(sicn_window::cut_plan(nullptr, &w8, &r, 3, nullptr, 1, nullptr, nullptr, nullptr, totals) == SICN_EINVAL);
    EXPECT(sicn_window::cut_plan(&w8, &w8, nullptr, 3, nullptr, 1, nullptr, nullptr, nullptr, totals) == SICN_EINVAL);
}

}  // namespace

int main()
{
    plans();
    bands();
    cuts();
    std::printf("window_plan_check ok: %d checks\n", checks);
    return 0;
}
