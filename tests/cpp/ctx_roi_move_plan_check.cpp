// Stand-alone check of csrc/ctx_roi_move_host.hpp (the stream and band capacities of a moving window of latent rows over a mode-4
// container, the placement of a position, the layout of the slots and the rows the placement writes) for builds with the host
// sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all ctx_roi_move_plan_check.cpp -o ctx_roi_move_plan_check
// Every output array lives in a heap block of EXACTLY its length, so a write past its end is an AddressSanitizer report, and the
// extreme coordinates make an overflowing sum an UndefinedBehaviorSanitizer report, not luck.  The rows of every placement are
// REPLAYED on heap blocks of exactly the layout's sizes: every byte the selected streams of both sets would write into the band, every
// neighbour the class rule would read there, and every byte the two cuts would read or write is touched.  Exit status 0 and one line
// "ctx_roi_move_plan_check ok: <n> checks" when everything held.  No device.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../simple_image_compression_network_amd/csrc/ctx_roi_move_host.hpp"

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

using namespace sicn_ctx_roi_move;

const int SIZES[][2] = {{592, 592}, {160, 640}, {48, 48}, {100, 36}, {16, 16}};
const int EXTREME[] = {INT_MIN, INT_MIN + 1, -100000, -16, -1, INT_MAX, INT_MAX - 1, 100000};

// pixel j of a set in raster order over row pairs (k_ctx_body.hpp ctx_pixel, restated)
void pixel(int set, uint64_t j, uint64_t W, uint64_t *y, uint64_t *x)
{
    const uint64_t a = (W + 1) / 2, b = W / 2, r = j / W, t = j - r * W;
    if (set == 0) {
        if (t < a) { *y = 2 * r; *x = 2 * t; } else { *y = 2 * r + 1; *x = 2 * (t - a) + 1; }
    } else {
        if (t < b) { *y = 2 * r; *x = 2 * t + 1; } else { *y = 2 * r + 1; *x = 2 * (t - b); }
    }
}

void capacities()
{
    const uint32_t lat[][3] = {{37, 37, 192}, {10, 40, 192}, {48, 40, 192}, {3, 3, 192}, {1, 5, 192}, {5, 1, 192}, {1, 1, 4}};
    for (auto &g : lat)
        for (uint32_t S : {1024u, 4096u, 16384u})
            for (uint32_t rh : {1u, 3u, 5u, g[1]}) {
                if (rh > g[1]) continue;
                auto cap = exact<uint32_t>(3);
                EXPECT(capacity(g[0], g[1], g[2], S, rh, cap.get()) == SICN_OK);
                uint32_t seen[3] = {0, 0, 0};
                for (uint32_t r0 = 0; r0 + rh <= g[1]; r0++) {
                    auto im = exact<sicn_ragged_ctx_window_image>(1);
                    EXPECT(sicn_ctx_window::plan_of_sl(g[0], g[1], g[2], S, r0, rh, 0, im.get()) == SICN_OK);
                    const uint32_t v[3] = {im[0].end_stream[0] - im[0].first_stream[0], im[0].end_stream[1] - im[0].first_stream[1], im[0].band_rows};
                    for (int k = 0; k < 3; k++) {
                        EXPECT(v[k] <= cap[k]);
                        if (v[k] > seen[k]) seen[k] = v[k];
                    }
                }
                EXPECT(seen[0] == cap[0] && seen[1] == cap[1] && seen[2] == cap[2]);       // exact maxima, not bounds
                if (g[0] == 1 && g[1] == 1) EXPECT(cap[0] == 1 && cap[1] == 0 && cap[2] == 1);
            }
    auto cap = exact<uint32_t>(3);
    EXPECT(capacity(37, 37, 192, 1024, 5, cap.get()) == SICN_OK && cap[0] == 50 && cap[1] == 22 && cap[2] == 18);
    EXPECT(capacity(7, 9, 192, 1024, 5, nullptr) == SICN_EINVAL && capacity(0, 9, 192, 1024, 5, cap.get()) == SICN_EINVAL);
    EXPECT(capacity(7, 9, 190, 1024, 5, cap.get()) == SICN_EINVAL && capacity(7, 9, 192, 1000, 5, cap.get()) == SICN_EINVAL);
    EXPECT(capacity(7, 9, 192, 1024, 0, cap.get()) == SICN_EINVAL && capacity(7, 9, 192, 1024, 10, cap.get()) == SICN_EINVAL);
    EXPECT(capacity(1u << 16, 1u << 16, 4, 1024, 1, cap.get()) == SICN_EINVAL && capacity(UINT_MAX, UINT_MAX, 4, 1024, UINT_MAX, cap.get()) == SICN_EINVAL);
}

// the rows of one placement, replayed: the decoder's writes into the band and the class rule's reads there, the latent cut and the
// pixel cut, on exact blocks
void replay(const SlotRow &s, const Placement &pl, const Totals &t, uint8_t *band, uint8_t *lat, uint8_t *recon, uint8_t *roi)
{
    const MoveRow &m = pl.win;
    const uint64_t W = (uint64_t)s.lat_w, H = (uint64_t)s.lat_h, C = s.lat_c, R = W * C, S = s.S;
    const uint64_t band_cap = (uint64_t)s.band_rows_cap * R;
    const uint64_t nsym[2] = {((H / 2) * W + ((H & 1) ? (W + 1) / 2 : 0)) * C, ((H / 2) * W + ((H & 1) ? W / 2 : 0)) * C};
    EXPECT(m.end[0] > m.first[0] && m.end[0] - m.first[0] <= s.max_streams[0] && m.end[1] - m.first[1] <= s.max_streams[1]);
    EXPECT(m.end[1] >= m.first[1] && pl.band_rows <= s.band_rows_cap && pl.band_rows >= (uint32_t)s.rh_cap);
    EXPECT(m.lat_bias + (uint64_t)pl.band_row0 * R == s.band_off);        // modulo 2^64, as the kernel adds it to the band's address
    uint64_t written = 0;
    for (int set = 0; set < 2; set++)
        for (uint64_t st = m.first[set]; st < m.end[set]; st++) {
            EXPECT(st * S < nsym[set]);
            const uint64_t begin = st * S, cnt = nsym[set] - begin < S ? nsym[set] - begin : S;
            EXPECT(begin % 4 == 0 && cnt % 4 == 0 && C % 4 == 0);
            for (uint64_t e = begin; e < begin + cnt; e += 4) {          // a lane's dword: 4 channels of one pixel
                uint64_t y, x;
                const uint64_t px = e / C, ch = e - px * C;
                pixel(set, px, W, &y, &x);
                const uint64_t at = m.lat_bias + (y * W + x) * C + ch;
                EXPECT(y >= pl.band_row0 && y < (uint64_t)pl.band_row0 + pl.band_rows);
                EXPECT(at >= s.band_off && at + 4 <= s.band_off + band_cap && at + 4 <= t.band);
                std::memset(band + at, 1 + set, 4);
                if (set == 1) {                                           // the four anchor neighbours the class rule gathers
                    if (y > 0) EXPECT(band[at - R] == 1);
                    if (y + 1 < H) EXPECT(band[at + R] == 1);
                    if (x > 0) EXPECT(band[at - C] == 1);
                    if (x + 1 < W) EXPECT(band[at + C] == 1);
                }
                written += 4;
            }
        }
    EXPECT(written == m.symbols);
    for (const CutRow *c : {&pl.lat_cut, &pl.pix_cut}) {
        const bool pix = c == &pl.pix_cut;
        const uint8_t *src = pix ? recon : band;
        uint8_t *dst = pix ? roi : lat;
        EXPECT(c->src_off >= 0 && c->dst_off >= 0);
        if (c->vec) EXPECT(((c->src_row | c->dst_row | c->src_off | c->dst_off) & 15) == 0);
        if (!pix) EXPECT((uint64_t)c->src_off >= s.band_off &&
                         (uint64_t)c->src_off + (uint64_t)(c->dst_h - 1) * c->src_row + c->dst_row <= s.band_off + (uint64_t)pl.band_rows * R);
        for (uint32_t y = 0; y < c->dst_h; y++) {
            std::memcpy(dst + c->dst_off + (size_t)y * c->dst_row, src + c->src_off + (size_t)y * c->src_row, c->dst_row);
            if (!pix)                                                     // every symbol of the window was decoded in this call
                for (uint32_t i = 0; i < c->dst_row; i++) EXPECT(dst[c->dst_off + (size_t)y * c->dst_row + i] != 0);
        }
    }
    EXPECT(pl.lat_cut.dst_h == (uint32_t)s.rh_cap && pl.lat_cut.dst_row == (uint32_t)s.cw_cap * s.lat_c);
    EXPECT(pl.pix_cut.dst_h == (uint32_t)s.h && pl.pix_cut.dst_row == (uint32_t)s.w * 3);
}

// one 112 x 144 image at 1024 symbols per stream, and what the refusals put in its place (namespace scope: default arguments name them)
const uint32_t lw = 7, lh = 9, iw = 112, ih = 144, wss = 1024, zero = 0, odd = 1000, wide = 113;

void layouts()
{
    for (uint32_t S : {1024u, 16384u}) {
        const int n_images = 5;
        const uint32_t lat_c = 192;
        const uint64_t coder_ws = 4096 * 7;
        auto lw = exact<uint32_t>(n_images), lh = exact<uint32_t>(n_images), iw = exact<uint32_t>(n_images), ih = exact<uint32_t>(n_images);   // shadow the constants above
        auto wl = exact<uint32_t>(n_images);
        for (int i = 0; i < n_images; i++) {
            iw[i] = SIZES[i][0]; ih[i] = SIZES[i][1]; lw[i] = (iw[i] + 15) / 16; lh[i] = (ih[i] + 15) / 16;
            wl[i] = S;
        }
        const sicn_ragged_roi_slot list[] = {{0, 20, 20}, {1, 33, 15}, {0, 256, 15}, {1, 17, 400}, {2, 16, 16}, {3, 33, 15}, {4, 16, 16}, {0, 20, 20},
                                             {1, 160, 640}, {3, 1, 1}};
        const int n_slots = (int)(sizeof list / sizeof list[0]);
        auto slots = exact<sicn_ragged_roi_slot>(n_slots);
        for (int k = 0; k < n_slots; k++) slots[k] = list[k];
        auto rows = exact<SlotRow>(n_slots);
        auto outs = exact<sicn_ragged_ctx_roi_move_slot>(n_slots);
        auto tot = exact<Totals>(1);
        EXPECT(layout(lw.get(), lh.get(), lat_c, wl.get(), iw.get(), ih.get(), coder_ws, n_images, slots.get(), n_slots, rows.get(), outs.get(),
                      tot.get()) == SICN_OK);
        const Totals t = tot[0];
        uint64_t band = 0, lat = 0, recon = 0, roi = 0, items[2] = {0, 0};
        for (int k = 0; k < n_slots; k++) {
            const SlotRow &s = rows[k];
            const int i = list[k].image;
            auto cap = exact<uint32_t>(3);
            EXPECT(capacity(lw[i], lh[i], lat_c, S, (uint32_t)s.rh_cap, cap.get()) == SICN_OK);
            EXPECT(s.max_streams[0] == cap[0] && s.max_streams[1] == cap[1] && s.band_rows_cap == cap[2]);
            EXPECT(s.band_off == band && band % 16 == 0 && s.lat_off == lat && s.recon_off == recon && s.roi_off == roi);
            EXPECT(s.meta_off == coder_ws + 64 * (uint64_t)k && s.first_item[0] == items[0] && s.first_item[1] == items[1] && s.image == (uint32_t)i);
            EXPECT(outs[k].band_offset == band && outs[k].latent_offset == lat && outs[k].recon_offset == recon && outs[k].roi_offset == roi &&
                   outs[k].meta_offset == s.meta_off && outs[k].max_streams[0] == cap[0] && outs[k].max_streams[1] == cap[1] &&
                   outs[k].band_rows_cap == cap[2] && outs[k].cw_cap == (uint32_t)s.cw_cap && outs[k].rh_cap == (uint32_t)s.rh_cap);
            EXPECT(outs[k].items[0] == (cap[0] + 7) / 8 && outs[k].items[1] == (cap[1] + 7) / 8);
            band += ((uint64_t)cap[2] * lw[i] * lat_c + 15) / 16 * 16;
            lat += (uint64_t)s.rh_cap * s.cw_cap * lat_c;
            recon += (uint64_t)s.rh_cap * s.cw_cap * 256 * 3;
            roi += (uint64_t)s.w * s.h * 3;
            items[0] += (cap[0] + 7) / 8;
            items[1] += (cap[1] + 7) / 8;
        }
        EXPECT(t.band == band && t.latent == lat && t.recon == recon && t.roi == roi && t.workspace == coder_ws + 64 * (uint64_t)n_slots);
        EXPECT(t.items[0] == items[0] && t.items[1] == items[1]);
        // every placement on a coarse grid and at the extremes, replayed on blocks of exactly the layout's sizes
        auto b_band = exact<uint8_t>(t.band), b_lat = exact<uint8_t>(t.latent), b_recon = exact<uint8_t>(t.recon), b_roi = exact<uint8_t>(t.roi);
        std::memset(b_recon.get(), 0, t.recon);
        for (int k = 0; k < n_slots; k++) {
            const SlotRow &s = rows[k];
            bool seen[3] = {false, false, false};
            std::vector<int> xs, ys;
            xs.push_back(-3); xs.push_back((s.image_w - s.w) / 2);
            for (int y = -3; y <= s.image_h - s.h + 3; y += 37) ys.push_back(y);
            for (int r = 0; r <= s.lat_h - s.rh_cap; r++) {              // every placed row is reached: r0 = floor((y0 - 15) / 16)
                const int y = 16 * r + 15;
                if (y <= s.image_h - s.h) ys.push_back(y);
            }
            for (int e : EXTREME) ys.push_back(e);
            xs.push_back(INT_MIN); xs.push_back(INT_MAX);
            xs.push_back(s.image_w - s.w); ys.push_back(s.image_h - s.h);
            for (int y0 : ys)
                for (int x0 : xs) {
                    auto pl = exact<Placement>(1);
                    auto p = exact<sicn_ragged_ctx_roi_placed>(1);
                    auto q = exact<sicn_ragged_roi_placed>(1);
                    pl[0] = place_slot(s, x0, y0);
                    EXPECT(place(s.image_w, s.image_h, s.lat_w, s.lat_h, s.lat_c, s.S, s.w, s.h, x0, y0, s.band_off, p.get()) == SICN_OK);
                    EXPECT(sicn_roi_move::place(UP, s.image_w, s.image_h, s.lat_w, s.lat_h, s.w, s.h, x0, y0, q.get()) == SICN_OK);
                    EXPECT(std::memcmp(&p[0].px, &q[0], sizeof q[0]) == 0 && pl[0].win.flags == q[0].flags);
                    EXPECT(p[0].lat_bias == pl[0].win.lat_bias && p[0].cut_offset == (uint64_t)pl[0].lat_cut.src_off);
                    EXPECT(p[0].first_stream[0] == pl[0].win.first[0] && p[0].end_stream[1] == pl[0].win.end[1] && p[0].symbols == pl[0].win.symbols);
                    const uint64_t R = (uint64_t)s.lat_w * s.lat_c;
                    EXPECT((uint64_t)pl[0].lat_cut.src_off == s.band_off + ((uint64_t)q[0].r0 - pl[0].band_row0) * R + (uint64_t)q[0].c0 * s.lat_c);
                    EXPECT((uint64_t)pl[0].pix_cut.src_off == s.recon_off + ((uint64_t)q[0].y * 16 * s.cw_cap + q[0].x) * 3);
                    std::memset(b_band.get() + s.band_off, 0, (size_t)s.band_rows_cap * R);       // the call's memset
                    replay(s, pl[0], t, b_band.get(), b_lat.get(), b_recon.get(), b_roi.get());
                    seen[0] |= pl[0].win.end[0] - pl[0].win.first[0] == s.max_streams[0];
                    seen[1] |= pl[0].win.end[1] - pl[0].win.first[1] == s.max_streams[1];
                    seen[2] |= pl[0].band_rows == s.band_rows_cap;
                }
            EXPECT(seen[0] && seen[1] && seen[2]);             // the capacities are met, not merely upper bounds
        }
    }
    // 64-bit offsets: 40 whole-height slots of 2^27 band bytes each (arithmetic only)
    {
        const uint32_t lw = 2048, lh = 16384, iw = 2048 * 16, ih = 16384 * 16, S = 16384;
        const int n_slots = 40;
        auto slots = exact<sicn_ragged_roi_slot>(n_slots);
        for (int k = 0; k < n_slots; k++) slots[k] = sicn_ragged_roi_slot{0, 16, 16384 * 16};
        auto outs = exact<sicn_ragged_ctx_roi_move_slot>(n_slots);
        auto tot = exact<Totals>(1);
        EXPECT(layout(&lw, &lh, 4, &S, &iw, &ih, 1 << 20, 1, slots.get(), n_slots, nullptr, outs.get(), tot.get()) == SICN_OK);
        EXPECT(outs[n_slots - 1].band_offset == (uint64_t)(n_slots - 1) << 27 && tot[0].band == (uint64_t)n_slots << 27);
        EXPECT(outs[n_slots - 1].max_streams[0] == 4096 && outs[n_slots - 1].max_streams[1] == 4096 && outs[n_slots - 1].band_rows_cap == 16384);
        auto p = exact<sicn_ragged_ctx_roi_placed>(1);
        EXPECT(place((int32_t)iw, (int32_t)ih, (int32_t)lw, (int32_t)lh, 4, S, 16, (int32_t)ih, INT_MAX, INT_MIN, outs[n_slots - 1].band_offset, p.get()) == SICN_OK);
        EXPECT(p[0].lat_bias == outs[n_slots - 1].band_offset && p[0].band_rows == 16384 && p[0].px.flags == SICN_ROI_MOVE_CLAMPED);
        EXPECT(p[0].cut_offset == outs[n_slots - 1].band_offset + (uint64_t)p[0].px.c0 * 4 && p[0].px.c0 == 2048 - 5);
    }
    // refusals
    {
        auto one = exact<sicn_ragged_roi_slot>(1);
        auto call = [&](sicn_ragged_roi_slot s, int n_slots = 1, int n_images = 1, const uint32_t *w = &wss, const uint32_t *image_w = &iw,
                        uint64_t wsb = 4096, uint32_t c = 192, const uint32_t *lat_w = &lw) {
            one[0] = s;
            return layout(lat_w, &lh, c, w, image_w, &ih, wsb, n_images, one.get(), n_slots, nullptr, nullptr, nullptr);
        };
        EXPECT(call({0, 20, 20}) == SICN_OK && call({0, 112, 144}) == SICN_OK && call({0, 20, 20}, 1, 1, nullptr) == SICN_OK);
        EXPECT(call({0, 0, 20}) == SICN_EINVAL && call({0, 20, 0}) == SICN_EINVAL && call({0, -5, 20}) == SICN_EINVAL);
        EXPECT(call({0, 113, 20}) == SICN_EINVAL && call({0, 20, 145}) == SICN_EINVAL && call({0, INT_MAX, INT_MAX}) == SICN_EINVAL);
        EXPECT(call({1, 20, 20}) == SICN_EINVAL && call({-1, 20, 20}) == SICN_EINVAL && call({INT_MAX, 20, 20}) == SICN_EINVAL);
        EXPECT(call({0, 20, 20}, 0) == SICN_EINVAL && call({0, 20, 20}, -1) == SICN_EINVAL && call({0, 20, 20}, 1, 0) == SICN_EINVAL);
        EXPECT(call({0, 20, 20}, 1, 1, &odd) == SICN_EINVAL && call({0, 20, 20}, 1, 1, &wss, &zero) == SICN_EINVAL);
        EXPECT(call({0, 20, 20}, 1, 1, &wss, &wide) == SICN_EINVAL && call({0, 20, 20}, 1, 1, &wss, &iw, 4100) == SICN_EINVAL);
        EXPECT(call({0, 20, 20}, 1, 1, &wss, &iw, 4096, 0) == SICN_EINVAL && call({0, 20, 20}, 1, 1, &wss, &iw, 4096, 190) == SICN_EINVAL);
        EXPECT(call({0, 20, 20}, 1, 1, &wss, &iw, 4096, 192, &zero) == SICN_EINVAL);
        EXPECT(layout(nullptr, &lh, 192, &wss, &iw, &ih, 4096, 1, one.get(), 1, nullptr, nullptr, nullptr) == SICN_EINVAL);
        EXPECT(layout(&lw, &lh, 192, &wss, &iw, &ih, 4096, 1, nullptr, 1, nullptr, nullptr, nullptr) == SICN_EINVAL);
        auto p = exact<sicn_ragged_ctx_roi_placed>(1);
        EXPECT(place(112, 144, 7, 9, 192, 1024, 1, 1, 0, 0, 0, nullptr) == SICN_EINVAL && place(112, 144, 7, 9, 192, 1024, 0, 1, 0, 0, 0, p.get()) == SICN_EINVAL);
        EXPECT(place(112, 144, 7, 9, 192, 1000, 1, 1, 0, 0, 0, p.get()) == SICN_EINVAL && place(112, 144, 7, 9, 190, 1024, 1, 1, 0, 0, 0, p.get()) == SICN_EINVAL);
        EXPECT(place(112, 144, 7, 9, 192, 1024, 1, 1, 0, 0, (uint64_t)1 << 62, p.get()) == SICN_EINVAL);
    }
}

}  // namespace

int main()
{
    capacities();
    layouts();
    std::printf("ctx_roi_move_plan_check ok: %lld checks\n", checks);
    return 0;
}
