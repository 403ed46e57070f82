// Stand-alone check of csrc/roi_move_host.hpp (the capacity of a moving ROI's latent window, the placement of a position, the layout
// of the slots and the rows the placement writes) for builds with the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all roi_move_plan_check.cpp -o roi_move_plan_check
// Every output array lives in a heap block of EXACTLY its length, so a write past its end is an AddressSanitizer report, and the
// extreme coordinates make an overflowing sum an UndefinedBehaviorSanitizer report, not luck.  The rows of every placement are
// REPLAYED on heap blocks of exactly the layout's sizes: every byte the window decoder would write and every byte the two cuts would
// read or write is touched.  Exit status 0 and one line "roi_move_plan_check ok: <n> checks" when everything held.  No device.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../simple_image_compression_network_amd/csrc/roi_move_host.hpp"

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

using namespace sicn_roi_move;

const int SIZES[][2] = {{112, 144}, {100, 131}, {16, 16}, {256, 48}, {64, 400}};
const int EXTREME[] = {INT_MIN, INT_MIN + 1, -100000, -16, -1, INT_MAX, INT_MAX - 1, 100000};

void placements()
{
    for (auto &sz : SIZES) {
        const int W = sz[0], H = sz[1], LW = (W + 15) / 16, LH = (H + 15) / 16;
        for (int w : {1, 15, 16, 17, 33, W})
            for (int h : {1, 16, 33, H}) {
                if (w > W || h > H) continue;
                auto cap = exact<int32_t>(2);
                EXPECT(capacity(4, W, H, LW, LH, w, h, cap.get()) == SICN_OK);
                EXPECT(cap[0] >= 1 && cap[0] <= LW && cap[0] <= (w + 75) / 16 && cap[1] >= 1 && cap[1] <= LH && cap[1] <= (h + 75) / 16);
                std::vector<int> xs, ys;
                for (int x = 0; x <= W - w; x += (x < 40 || x > W - w - 40) ? 1 : 7) xs.push_back(x);
                for (int y = 0; y <= H - h; y += (y < 20 || y > H - h - 20) ? 1 : 13) ys.push_back(y);
                for (int x0 : xs)
                    for (int y0 : ys) {
                        auto p = exact<sicn_ragged_roi_placed>(1);
                        auto plan = exact<sicn_ragged_roi>(1);
                        const sicn_ragged_rect r{x0, y0, w, h};
                        EXPECT(place(4, W, H, LW, LH, w, h, x0, y0, p.get()) == SICN_OK);
                        EXPECT(sicn_window::roi_plan(4, W, H, LW, LH, &r, plan.get()) == SICN_OK);
                        EXPECT(p[0].flags == 0 && p[0].x0 == x0 && p[0].y0 == y0 && p[0].cw == cap[0] && p[0].rh == cap[1]);
                        EXPECT(p[0].c0 >= 0 && p[0].c0 + p[0].cw <= LW && p[0].r0 >= 0 && p[0].r0 + p[0].rh <= LH);
                        EXPECT(p[0].c0 <= plan[0].c0 && p[0].c0 + p[0].cw >= plan[0].c0 + plan[0].cw);
                        EXPECT(p[0].r0 <= plan[0].r0 && p[0].r0 + p[0].rh >= plan[0].r0 + plan[0].rh);
                        EXPECT(plan[0].c0 != 0 || p[0].c0 == 0);
                        EXPECT(plan[0].c0 + plan[0].cw != LW || p[0].c0 + p[0].cw == LW);
                        EXPECT(p[0].x == x0 - 16 * p[0].c0 && p[0].y == y0 - 16 * p[0].r0);
                        EXPECT(p[0].x >= 0 && p[0].x + w <= 16 * p[0].cw && p[0].y >= 0 && p[0].y + h <= 16 * p[0].rh);
                    }
                for (int e : EXTREME)
                    for (int other : {0, 5, INT_MAX, INT_MIN}) {
                        auto p = exact<sicn_ragged_roi_placed>(1), q = exact<sicn_ragged_roi_placed>(1);
                        EXPECT(place(4, W, H, LW, LH, w, h, e, other, p.get()) == SICN_OK);
                        const int cx = e < 0 ? 0 : W - w, cy = other < 0 ? 0 : other > H - h ? H - h : other;
                        EXPECT(p[0].flags == SICN_ROI_MOVE_CLAMPED && p[0].x0 == cx && p[0].y0 == cy);
                        EXPECT(place(4, W, H, LW, LH, w, h, cx, cy, q.get()) == SICN_OK && q[0].flags == 0);
                        EXPECT(p[0].c0 == q[0].c0 && p[0].r0 == q[0].r0 && p[0].x == q[0].x && p[0].y == q[0].y);
                    }
            }
    }
    // other layer counts, and the largest sizes
    for (int l = 1; l <= sicn_window::MAX_UP_LAYERS; l++) {
        int64_t lo = 0, hi = 0;
        for (int k = 0; k < l; k++) { lo = 2 * lo + 1; hi = 2 * hi + 2; }      // the recurrences of include/sicn_ragged_window.h
        EXPECT(lo == margin_lo(l) && hi == margin_hi(l));
        auto p = exact<sicn_ragged_roi_placed>(1);
        const int lat = 1 << 20 >> (l > 10 ? l - 10 : 0), image = (int)(((int64_t)lat << l) > INT_MAX ? INT_MAX : (int64_t)lat << l);
        EXPECT(place(l, image, image, lat, lat, image, 1, INT_MAX, INT_MAX, p.get()) == SICN_OK);
        EXPECT(p[0].x0 == 0 && p[0].y0 == image - 1 && p[0].cw == lat && p[0].r0 + p[0].rh == lat);
    }
}

void refusals()
{
    auto cap = exact<int32_t>(2);
    auto p = exact<sicn_ragged_roi_placed>(1);
    EXPECT(capacity(4, 112, 144, 7, 9, 20, 20, cap.get()) == SICN_OK);
    EXPECT(capacity(4, 112, 144, 7, 9, 0, 20, cap.get()) == SICN_EINVAL && capacity(4, 112, 144, 7, 9, 20, 0, cap.get()) == SICN_EINVAL);
    EXPECT(capacity(4, 112, 144, 7, 9, -1, 20, cap.get()) == SICN_EINVAL && capacity(4, 112, 144, 7, 9, INT_MIN, 20, cap.get()) == SICN_EINVAL);
    EXPECT(capacity(4, 112, 144, 7, 9, 113, 20, cap.get()) == SICN_EINVAL && capacity(4, 112, 144, 7, 9, 20, 145, cap.get()) == SICN_EINVAL);
    EXPECT(capacity(4, 112, 144, 7, 9, INT_MAX, INT_MAX, cap.get()) == SICN_EINVAL);
    EXPECT(capacity(4, 113, 144, 7, 9, 20, 20, cap.get()) == SICN_EINVAL && capacity(4, 112, 145, 7, 9, 20, 20, cap.get()) == SICN_EINVAL);
    EXPECT(capacity(4, 0, 144, 7, 9, 1, 1, cap.get()) == SICN_EINVAL && capacity(4, 112, 144, 0, 9, 1, 1, cap.get()) == SICN_EINVAL);
    EXPECT(capacity(0, 112, 144, 7, 9, 1, 1, cap.get()) == SICN_EINVAL && capacity(13, 112, 144, 7, 9, 1, 1, cap.get()) == SICN_EINVAL);
    EXPECT(capacity(4, 112, 144, 7, 9, 1, 1, nullptr) == SICN_EINVAL);
    EXPECT(place(4, 112, 144, 7, 9, 1, 1, 0, 0, nullptr) == SICN_EINVAL && place(4, 112, 144, 7, 9, 0, 1, 0, 0, p.get()) == SICN_EINVAL);
}

// the rows of one placement, replayed: the decoder's writes into the band, the latent cut and the pixel cut, on exact blocks
void replay(const SlotRow &s, const Placement &pl, const Totals &t, uint8_t *band, uint8_t *lat, uint8_t *recon, uint8_t *roi)
{
    const MoveRow &m = pl.win;
    EXPECT(m.end_stream > m.first_stream && m.end_stream - m.first_stream <= s.max_streams);
    EXPECT((uint64_t)m.end_stream * s.wss < (uint64_t)s.n + s.wss);
    uint64_t written = 0;
    for (uint32_t st = m.first_stream; st < m.end_stream; st++) {
        const uint64_t begin = (uint64_t)st * s.wss, cnt = s.n - begin < s.wss ? s.n - begin : s.wss;
        const uint64_t at = m.lat_bias + begin;              // modulo 2^64, as the kernel adds it to the band's address
        EXPECT(at >= s.band_off && at + cnt <= s.band_off + (uint64_t)s.max_streams * s.wss && at + cnt <= t.band);
        std::memset(band + at, 1, cnt);
        written += cnt;
    }
    EXPECT(written == m.symbols);
    for (const CutRow *c : {&pl.lat_cut, &pl.pix_cut}) {
        const bool pix = c == &pl.pix_cut;
        const uint8_t *src = pix ? recon : band;
        uint8_t *dst = pix ? roi : lat;
        EXPECT(c->src_off >= 0 && c->dst_off >= 0);
        if (c->vec) EXPECT(((c->src_row | c->dst_row | c->src_off | c->dst_off) & 15) == 0);
        if (!pix) EXPECT((uint64_t)c->src_off >= s.band_off && (uint64_t)c->src_off + (uint64_t)(c->dst_h - 1) * c->src_row + c->dst_row <=
                                                                    (m.lat_bias + (uint64_t)m.first_stream * s.wss) + m.symbols);
        for (uint32_t y = 0; y < c->dst_h; y++)
            std::memcpy(dst + c->dst_off + (size_t)y * c->dst_row, src + c->src_off + (size_t)y * c->src_row, c->dst_row);
    }
    EXPECT(pl.lat_cut.dst_h == (uint32_t)s.rh_cap && pl.lat_cut.dst_row == (uint32_t)s.cw_cap * s.lat_c);
    EXPECT(pl.pix_cut.dst_h == (uint32_t)s.h && pl.pix_cut.dst_row == (uint32_t)s.w * 3);
}

// one 112 x 144 image at 1024 symbols per stream, and what the refusals put in its place (namespace scope: default arguments name them)
const uint32_t lw = 7, lh = 9, iw = 112, ih = 144, wss = 1024, zero = 0, odd = 1000, wide = 113;
const uint64_t ws = 4096, ws_odd = 4100;

void layouts()
{
    for (uint32_t wss : {1024u, 4096u, 16384u}) {       // shadows the constant above
        const int n_images = 5;
        const uint32_t lat_c = 192;
        auto lw = exact<uint32_t>(n_images), lh = exact<uint32_t>(n_images), iw = exact<uint32_t>(n_images), ih = exact<uint32_t>(n_images);
        auto wl = exact<uint32_t>(n_images);
        auto ws = exact<uint64_t>(n_images);
        for (int i = 0; i < n_images; i++) {
            iw[i] = SIZES[i][0]; ih[i] = SIZES[i][1]; lw[i] = (iw[i] + 15) / 16; lh[i] = (ih[i] + 15) / 16;
            wl[i] = wss; ws[i] = 256 * (uint64_t)(i + 3);
        }
        const sicn_ragged_roi_slot list[] = {{0, 20, 20}, {4, 64, 33}, {0, 1, 1}, {3, 256, 48}, {2, 16, 16}, {1, 100, 15}, {0, 112, 1}, {4, 17, 400},
                                             {0, 20, 20}, {1, 33, 15}};
        const int n_slots = (int)(sizeof list / sizeof list[0]);
        auto slots = exact<sicn_ragged_roi_slot>(n_slots);
        for (int k = 0; k < n_slots; k++) slots[k] = list[k];
        auto rows = exact<SlotRow>(n_slots);
        auto outs = exact<sicn_ragged_roi_move_slot>(n_slots);
        auto tot = exact<Totals>(1);
        EXPECT(layout(lw.get(), lh.get(), lat_c, wl.get(), iw.get(), ih.get(), ws.get(), n_images, slots.get(), n_slots, rows.get(), outs.get(),
                      tot.get()) == SICN_OK);
        const Totals t = tot[0];
        uint64_t band = 0, lat = 0, recon = 0, roi = 0, wsp = 0, items = 0;
        for (int k = 0; k < n_slots; k++) {
            const SlotRow &s = rows[k];
            const int i = list[k].image;
            const uint64_t R = (uint64_t)lw[i] * lat_c, n = R * lh[i], ns = (n + wss - 1) / wss;
            uint64_t ms = ((uint64_t)s.rh_cap * R + wss - 1) / wss + 1;
            if (ms > ns) ms = ns;
            EXPECT(s.max_streams == ms && s.band_off == band && band % 16 == 0 && s.lat_off == lat && s.recon_off == recon && s.roi_off == roi);
            EXPECT(s.ws_off == wsp && s.first_item == items && s.image == (uint32_t)i && s.n == n);
            EXPECT(outs[k].band_offset == band && outs[k].latent_offset == lat && outs[k].recon_offset == recon && outs[k].roi_offset == roi &&
                   outs[k].workspace_offset == wsp && outs[k].max_streams == ms && outs[k].first_item == items &&
                   outs[k].cw_cap == (uint32_t)s.cw_cap && outs[k].rh_cap == (uint32_t)s.rh_cap);
            band += (ms * wss + 15) / 16 * 16;
            lat += (uint64_t)s.rh_cap * s.cw_cap * lat_c;
            recon += (uint64_t)s.rh_cap * s.cw_cap * 256 * 3;
            roi += (uint64_t)s.w * s.h * 3;
            wsp += ws[i];
            items += ms;
        }
        EXPECT(t.band == band && t.latent == lat && t.recon == recon && t.roi == roi && t.workspace == wsp && t.items == items);
        if (wss == 1024) EXPECT(rows[0].max_streams == 8 && rows[0].rh_cap == 5);      // a 20 x 20 slot of 112 x 144: at most 8 of 12 streams
        // every placement on a coarse grid and at the extremes, replayed on blocks of exactly the layout's sizes
        auto b_band = exact<uint8_t>(t.band), b_lat = exact<uint8_t>(t.latent), b_recon = exact<uint8_t>(t.recon), b_roi = exact<uint8_t>(t.roi);
        std::memset(b_band.get(), 0, t.band);
        std::memset(b_recon.get(), 0, t.recon);
        for (int k = 0; k < n_slots; k++) {
            const SlotRow &s = rows[k];
            bool seen_max = false;
            std::vector<int> xs, ys;
            for (int x = -3; x <= s.image_w - s.w + 3; x += 5) xs.push_back(x);
            for (int y = -3; y <= s.image_h - s.h + 3; y += 1) ys.push_back(y);
            for (int e : EXTREME) { xs.push_back(e); ys.push_back(e); }
            xs.push_back(s.image_w - s.w); ys.push_back(s.image_h - s.h);
            for (int x0 : xs)
                for (int y0 : ys) {
                    auto pl = exact<Placement>(1);
                    auto p = exact<sicn_ragged_roi_placed>(1);
                    pl[0] = place_slot(s, x0, y0);
                    EXPECT(place(UP, s.image_w, s.image_h, s.lat_w, s.lat_h, s.w, s.h, x0, y0, p.get()) == SICN_OK);
                    EXPECT(pl[0].win.flags == p[0].flags);
                    const uint64_t R = (uint64_t)s.lat_w * s.lat_c;
                    EXPECT(pl[0].win.first_stream == (uint64_t)p[0].r0 * R / wss);
                    EXPECT((uint64_t)pl[0].lat_cut.src_off == s.band_off + ((uint64_t)p[0].r0 * R - (uint64_t)pl[0].win.first_stream * wss) +
                                                                  (uint64_t)p[0].c0 * s.lat_c);
                    EXPECT((uint64_t)pl[0].pix_cut.src_off == s.recon_off + ((uint64_t)p[0].y * 16 * s.cw_cap + p[0].x) * 3);
                    replay(s, pl[0], t, b_band.get(), b_lat.get(), b_recon.get(), b_roi.get());
                    seen_max |= pl[0].win.end_stream - pl[0].win.first_stream == s.max_streams;
                }
            EXPECT(seen_max);                              // the capacity is met, not merely an upper bound
        }
    }
    // 64-bit offsets: 140 slots of 2^25 band bytes each (arithmetic only)
    {
        const uint32_t lw = 4096, lh = 8192, iw = 65536, ih = 131072, wss = 16384;      // shadow the constants above
        const uint64_t ws = 1 << 20;
        const int n_slots = 140;
        auto slots = exact<sicn_ragged_roi_slot>(n_slots);
        for (int k = 0; k < n_slots; k++) slots[k] = sicn_ragged_roi_slot{0, 16, 131072};
        auto outs = exact<sicn_ragged_roi_move_slot>(n_slots);
        auto tot = exact<Totals>(1);
        EXPECT(layout(&lw, &lh, 1, &wss, &iw, &ih, &ws, 1, slots.get(), n_slots, nullptr, outs.get(), tot.get()) == SICN_OK);
        EXPECT(outs[n_slots - 1].band_offset == (uint64_t)(n_slots - 1) << 25 && tot[0].band == (uint64_t)n_slots << 25);
        EXPECT(outs[n_slots - 1].max_streams == 2048 && outs[n_slots - 1].cw_cap == 5 && outs[n_slots - 1].rh_cap == 8192);
        slots[n_slots - 1] = sicn_ragged_roi_slot{0, 65536, 131072};       // a reconstruction of 2^31 bytes and more
        EXPECT(layout(&lw, &lh, 1, &wss, &iw, &ih, &ws, 1, slots.get(), n_slots, nullptr, nullptr, nullptr) == SICN_EINVAL);
    }
    // refusals
    {
        auto one = exact<sicn_ragged_roi_slot>(1);
        auto call = [&](sicn_ragged_roi_slot s, int n_slots = 1, int n_images = 1, const uint32_t *w = &wss, const uint32_t *image_w = &iw,
                        const uint64_t *wsb = &ws, uint32_t c = 192, const uint32_t *lat_w = &lw) {
            one[0] = s;
            return layout(lat_w, &lh, c, w, image_w, &ih, wsb, n_images, one.get(), n_slots, nullptr, nullptr, nullptr);
        };
        EXPECT(call({0, 20, 20}) == SICN_OK && call({0, 112, 144}) == SICN_OK && call({0, 20, 20}, 1, 1, nullptr) == SICN_OK);
        EXPECT(call({0, 0, 20}) == SICN_EINVAL && call({0, 20, 0}) == SICN_EINVAL && call({0, -5, 20}) == SICN_EINVAL);
        EXPECT(call({0, 113, 20}) == SICN_EINVAL && call({0, 20, 145}) == SICN_EINVAL && call({0, INT_MAX, INT_MAX}) == SICN_EINVAL);
        EXPECT(call({1, 20, 20}) == SICN_EINVAL && call({-1, 20, 20}) == SICN_EINVAL && call({INT_MAX, 20, 20}) == SICN_EINVAL);
        EXPECT(call({0, 20, 20}, 0) == SICN_EINVAL && call({0, 20, 20}, -1) == SICN_EINVAL && call({0, 20, 20}, 1, 0) == SICN_EINVAL);
        EXPECT(call({0, 20, 20}, 1, 1, &odd) == SICN_EINVAL && call({0, 20, 20}, 1, 1, &wss, &zero) == SICN_EINVAL);
        EXPECT(call({0, 20, 20}, 1, 1, &wss, &wide) == SICN_EINVAL && call({0, 20, 20}, 1, 1, &wss, &iw, &ws_odd) == SICN_EINVAL);
        EXPECT(call({0, 20, 20}, 1, 1, &wss, &iw, &ws, 0) == SICN_EINVAL && call({0, 20, 20}, 1, 1, &wss, &iw, &ws, 192, &zero) == SICN_EINVAL);
        EXPECT(layout(nullptr, &lh, 192, &wss, &iw, &ih, &ws, 1, one.get(), 1, nullptr, nullptr, nullptr) == SICN_EINVAL);
        EXPECT(layout(&lw, &lh, 192, &wss, &iw, &ih, nullptr, 1, one.get(), 1, nullptr, nullptr, nullptr) == SICN_EINVAL);
        EXPECT(layout(&lw, &lh, 192, &wss, &iw, &ih, &ws, 1, nullptr, 1, nullptr, nullptr, nullptr) == SICN_EINVAL);
        const uint32_t big_w = 2049, big_h = 1024, big_iw = 2049 * 16, big_ih = 1024 * 16;      // more than 2048 streams
        one[0] = sicn_ragged_roi_slot{0, 20, 20};
        EXPECT(layout(&big_w, &big_h, 1, &wss, &big_iw, &big_ih, &ws, 1, one.get(), 1, nullptr, nullptr, nullptr) == SICN_EINVAL);
    }
}

}  // namespace

int main()
{
    placements();
    refusals();
    layouts();
    std::printf("roi_move_plan_check ok: %lld checks\n", checks);
    return 0;
}
