// Stand-alone check of csrc/ragged_rect_host.hpp (the rectangle epilogue of the packed deconv N -> 3 of a ragged net,
// include/sicn_ragged_rect.h) for builds with the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all ragged_rect_check.cpp -o ragged_rect_check
// For small reconstructions, several rectangle sizes and EVERY origin in a margin around the reconstruction — and at INT32_MIN /
// INT32_MAX — the kernel's walk is replayed: every tile of the deconv's grid is put to the tile test, every lane of every tile that
// passes to the store predicate, and what is stored goes into a heap block of EXACTLY 3 h w bytes at the address the header gives
// (the sanitizers see any other address, and any signed overflow on the way).  Then, in both layouts:
//   - every pixel of the rectangle that lies inside the reconstruction was stored exactly once, with the value of its own
//     reconstruction pixel, where direct indexing of [h][w][3] / [3][h][w] finds it
//   - nothing else was stored
//   - a tile that failed the test holds no pixel the predicate would store
// Exit status 0 and one line "ragged_rect_check ok: <n> checks" when everything held.  No device, no library.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../simple_image_compression_network_amd/csrc/ragged_rect_host.hpp"

namespace {

using namespace sicn;

long long checks = 0;

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        checks++;                                                                     \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

constexpr int TILE = 16;      // rgb_deconv_tile (csrc/k_rgb_ragged_body.hpp): 16 x 16 input positions, four phases each

struct Size {
    int w, h;
};

uint8_t value(int ch, int y, int x) { return (uint8_t)(1 + ch * 89 + y * 7 + x * 3); }

long long stored_total = 0, skipped_total = 0;

template <bool PLANAR>
void check_rect(Size in, int32_t x0, int32_t y0, int w, int h)
{
    const int IW = in.w, IH = in.h, RW = 2 * IW, RH = 2 * IH;
    const size_t bytes = 3 * (size_t)w * h;
    std::unique_ptr<uint8_t[]> count(new uint8_t[bytes]), vals(new uint8_t[bytes]);     // exactly the image's own bytes
    std::memset(count.get(), 0, bytes);
    std::memset(vals.get(), 0, bytes);
    for (int ty0 = 0; ty0 < IH; ty0 += TILE)
        for (int tx0 = 0; tx0 < IW; tx0 += TILE) {
            const bool live = rect_tile_live(ty0, tx0, x0, y0, w, h);
            if (!live) skipped_total++;
            for (int wv = 0; wv < 4; wv++)
                for (int lane = 0; lane < 64; lane++)
                    for (int c = 0; c < 4; c++) {
                        const int col = lane & 15, g = lane >> 4;
                        const int oy = 2 * (ty0 + 4 * wv + c) + (g >> 1), ox = 2 * (tx0 + col) + (g & 1);
                        const bool st = rect_stored(oy, ox, RW, RH, x0, y0, w, h);
                        if (!live) {
                            EXPECT(!st);                                  // a skipped tile holds no stored pixel
                            continue;
                        }
                        if (!st) continue;
                        const uint32_t ry = rect_rel(oy, y0), rx = rect_rel(ox, x0);
                        EXPECT((int64_t)ry == (int64_t)oy - y0 && (int64_t)rx == (int64_t)ox - x0);
                        for (int ch = 0; ch < 3; ch++) {
                            const int64_t at = rect_at<PLANAR>(ch, ry, rx, w, h);
                            EXPECT(at >= 0 && at < (int64_t)bytes);
                            count[(size_t)at]++;
                            vals[(size_t)at] = value(ch, oy, ox);
                            stored_total++;
                        }
                    }
        }
    // direct indexing: byte (ch, y, x) of the rectangle is reconstruction pixel (y0 + y, x0 + x) where that exists, untouched elsewhere
    for (int ch = 0; ch < 3; ch++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t at = PLANAR ? ((size_t)ch * h + y) * w + x : ((size_t)y * w + x) * 3 + ch;
                const int64_t oy = (int64_t)y0 + y, ox = (int64_t)x0 + x;
                const bool inside = oy >= 0 && oy < RH && ox >= 0 && ox < RW;
                EXPECT(count[at] == (inside ? 1 : 0));
                if (inside) EXPECT(vals[at] == value(ch, (int)oy, (int)ox));
            }
}

void check_both(Size in, int32_t x0, int32_t y0, int w, int h)
{
    check_rect<false>(in, x0, y0, w, h);
    check_rect<true>(in, x0, y0, w, h);
}

}  // namespace

int main()
{
    // input maps: one tile, tile edges at 15 / 16 / 17, more than one tile both ways
    const std::vector<Size> maps = {{1, 1}, {16, 16}, {17, 15}, {33, 2}, {2, 33}, {20, 18}};
    const int32_t extremes[] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX};
    for (const Size &in : maps) {
        const int RW = 2 * in.w, RH = 2 * in.h;
        const std::vector<Size> rects = {{1, 1}, {RW, RH}, {3, 5}, {33, 31}, {RW > 1 ? RW - 1 : 1, 2}};
        for (const Size &r : rects) {
            // every origin in a margin around the reconstruction: from where the rectangle just misses it on one side to where it
            // just misses it on the other
            const int m = 3;
            for (int y0 = -r.h - m; y0 <= RH + m; y0++)
                for (int x0 = -r.w - m; x0 <= RW + m; x0++) check_both(in, x0, y0, r.w, r.h);
            for (int32_t ey : extremes)
                for (int32_t ex : extremes) check_both(in, ex, ey, r.w, r.h);
        }
    }
    EXPECT(stored_total > 0 && skipped_total > 0);
    std::printf("ragged_rect_check ok: %lld checks\n", checks);
    return 0;
}
