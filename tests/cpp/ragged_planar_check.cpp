// Stand-alone check of csrc/ragged_planar_host.hpp (the loader arithmetic of the planar conv 3 -> N and the store arithmetic of the
// planar deconv N -> 3 of a ragged net, include/sicn_ragged_planar.h) for builds with the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all ragged_planar_check.cpp -o ragged_planar_check
// The loader: batches of small planar images lie back to back in a heap block of EXACTLY the permitted size — the tensor rounded up
// to a multiple of 4 — and planar_quad, the function the kernel calls, is run for every quad of every tile of every image as the
// kernel's loop runs it.  Every load must be an aligned dword inside the block (the sanitizer sees any other), the assembled RGBX
// dwords must equal direct indexing, and the batches must bring the start of each of the three planes and the starts of the rows
// to all four byte phases.  The store: every lane of every tile of the deconv's grid, for cuts to (1, 1), (OW - 1, OH),
// (OW, OH - 1) and the full size — each byte of each cut image is written exactly once and nothing else is.
// Exit status 0 and one line "ragged_planar_check ok: <n> checks" when everything held.  No device, no library.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../simple_image_compression_network_amd/csrc/ragged_planar_host.hpp"

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

// the geometry of rgb_conv_tile / rgb_deconv_tile (csrc/k_rgb_ragged_body.hpp): 16 x 16 tiles; a conv patch of 36 rows of 10 quads
// from input pixel (2 y0 - 2, 2 x0 - 2) on
constexpr int TILE = 16, PATCH_ROWS = 36, ROW_QUADS = 10;

struct Size {
    int w, h;
};

std::mt19937 rng(20261021u);

// ---- the loader ---------------------------------------------------------------------------------------------------------------------
struct Coverage {
    bool plane[3][4] = {}, row[4] = {};
    bool all() const
    {
        for (int p = 0; p < 4; p++) {
            if (!row[p]) return false;
            for (int c = 0; c < 3; c++)
                if (!plane[c][p]) return false;
        }
        return true;
    }
};

void check_loader(const std::vector<Size> &batch, Coverage *cov)
{
    std::vector<int64_t> off(batch.size() + 1, 0);
    for (size_t i = 0; i < batch.size(); i++) off[i + 1] = off[i] + 3ll * batch[i].w * batch[i].h;
    const size_t total = (size_t)off.back(), permitted = (total + 3) & ~(size_t)3;
    std::unique_ptr<uint8_t[]> block(new uint8_t[permitted]);          // operator new: aligned to more than 4
    uint8_t *t = block.get();
    EXPECT(((uintptr_t)t & 3) == 0);
    for (size_t i = 0; i < permitted; i++) t[i] = (uint8_t)(1u + rng() % 255u);     // never 0: a zero must come from the loader
    const uintptr_t lo = (uintptr_t)t, hi = lo + total;
    long long loads = 0;
    auto load = [&](uintptr_t a) {
        EXPECT((a & 3) == 0 && a >= lo && a + 4 <= lo + permitted);    // inside [t0, round4(t1))
        EXPECT(a + 4 > lo && a < hi);                                  // and it overlaps the tensor
        loads++;
        uint32_t v;
        std::memcpy(&v, reinterpret_cast<const void *>(a), 4);
        return v;
    };
    for (size_t i = 0; i < batch.size(); i++) {
        const int W = batch[i].w, H = batch[i].h;
        const uint8_t *im = t + off[i];
        for (int c = 0; c < 3; c++) cov->plane[c][(off[i] + planar_at(c, 0, 0, W, H)) & 3] = true;
        for (int c = 0; c < 3; c++)
            for (int y = 0; y < H; y++) cov->row[(off[i] + planar_at(c, y, 0, W, H)) & 3] = true;
        const int OW = (W + 1) / 2, OH = (H + 1) / 2;
        for (int y0 = 0; y0 < OH; y0 += TILE)
            for (int x0 = 0; x0 < OW; x0 += TILE)
                for (int r = 0; r < PATCH_ROWS; r++)
                    for (int gq = 0; gq < ROW_QUADS; gq++) {
                        const int iy = 2 * y0 - 2 + r, ix = 2 * x0 - 2 + 4 * gq;
                        const PlanarQuad q = planar_quad((uintptr_t)im, W, H, iy, ix, lo, hi, load);
                        for (int k = 0; k < 4; k++) {
                            const int x = ix + k;
                            uint32_t want = 0;
                            if (iy >= 0 && iy < H && x >= 0 && x < W)
                                want = (uint32_t)im[planar_at(0, iy, x, W, H)] | (uint32_t)im[planar_at(1, iy, x, W, H)] << 8 |
                                       (uint32_t)im[planar_at(2, iy, x, W, H)] << 16;
                            EXPECT(q.px[k] == want);
                        }
                    }
    }
    EXPECT(loads > 0);
}

// ---- the store ----------------------------------------------------------------------------------------------------------------------
void check_store(const std::vector<Size> &inputs, int which_cut)
{
    std::vector<PlanarOut> cuts;
    int64_t total = 0;
    for (const Size &s : inputs) {
        const int OW = 2 * s.w, OH = 2 * s.h;
        Size c = {OW, OH};
        if (which_cut == 0) c = {1, 1};
        if (which_cut == 1 && OW > 1) c = {OW - 1, OH};
        if (which_cut == 2 && OH > 1) c = {OW, OH - 1};
        cuts.push_back(PlanarOut{c.w, c.h, total});
        total += 3ll * c.w * c.h;
    }
    std::unique_ptr<uint8_t[]> block(new uint8_t[(size_t)total]);     // exactly the tensor: a store outside is the sanitizer's
    std::memset(block.get(), 0, (size_t)total);
    std::vector<uint8_t> vals((size_t)total, 0);                      // what the lane stored: a value of (plane, row, column)
    auto value = [](int ch, int y, int x) { return (uint8_t)(1 + ch * 89 + y * 7 + x * 3); };
    for (size_t i = 0; i < inputs.size(); i++) {
        const int IW = inputs[i].w, IH = inputs[i].h, w = cuts[i].w, h = cuts[i].h;
        uint8_t *om = block.get() + cuts[i].off;
        for (int y0 = 0; y0 < IH; y0 += TILE)
            for (int x0 = 0; x0 < IW; x0 += TILE)
                for (int wv = 0; wv < 4; wv++)
                    for (int lane = 0; lane < 64; lane++)
                        for (int c = 0; c < 4; c++) {
                            const int col = lane & 15, g = lane >> 4;
                            const int oy = 2 * (y0 + 4 * wv + c) + (g >> 1), ox = 2 * (x0 + col) + (g & 1);
                            if (!planar_stored(oy, ox, w, h)) continue;
                            EXPECT(oy < 2 * IH && ox < 2 * IW);                  // a stored pixel is one the tile computed
                            for (int ch = 0; ch < 3; ch++) {
                                const int64_t at = planar_at(ch, oy, ox, w, h);
                                EXPECT(at >= 0 && at < 3ll * w * h);
                                om[at]++;
                                vals[(size_t)(cuts[i].off + at)] = value(ch, oy, ox);
                            }
                        }
    }
    for (int64_t k = 0; k < total; k++) EXPECT(block[(size_t)k] == 1);           // every byte once, none twice
    // and each where direct indexing of [3][h][w] finds it
    for (size_t i = 0; i < inputs.size(); i++) {
        const uint8_t *img = vals.data() + cuts[i].off;
        size_t k = 0;
        for (int ch = 0; ch < 3; ch++)
            for (int y = 0; y < cuts[i].h; y++)
                for (int x = 0; x < cuts[i].w; x++) EXPECT(img[k++] == value(ch, y, x));
    }
}

}  // namespace

int main()
{
    const int widths[] = {1, 2, 3, 4, 5, 31, 32, 33, 35}, heights[] = {1, 2, 3, 33};
    // every width with every height, in three orders: the offsets before an image, and so its phases, differ between them
    std::vector<Size> all;
    for (int h : heights)
        for (int w : widths) all.push_back(Size{w, h});
    Coverage cov;
    check_loader(all, &cov);
    std::vector<Size> reversed(all.rbegin(), all.rend());
    check_loader(reversed, &cov);
    std::vector<Size> shuffled = all;
    std::shuffle(shuffled.begin(), shuffled.end(), rng);
    check_loader(shuffled, &cov);
    // one image alone: the tensor begins and ends with it, at every size
    for (const Size &s : all) check_loader({s}, &cov);
    EXPECT(cov.all());

    // the deconv's input maps: tile edges at 15 / 16 / 17, more than one tile both ways
    const std::vector<Size> maps = {{1, 1}, {16, 16}, {17, 15}, {33, 2}, {2, 33}, {50, 18}};
    for (int cut = 0; cut < 4; cut++) check_store(maps, cut);

    std::printf("ragged_planar_check ok: %lld checks\n", checks);
    return 0;
}
