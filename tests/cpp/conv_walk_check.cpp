// The K walk of the wide persistent conv (csrc/conv_walk.hpp) replayed on the host, pass by pass, for tiles over NG = 3 and 4 channel
// groups: three consecutive tiles of one workgroup.  Nothing here asks schedule_ok() / schedule3_ok(): the replay keeps, for every
// 4 KiB piece of the four planes and every slot of the weight ring, WHAT it holds (tile, group / stream step) and in which pass that
// was requested, does to this state what a pass of the kernel does (k_mfma16x_body.hpp: conv_pass_x — the reads of the NEXT pass's
// fragments and this pass's requests run side by side, then the counted wait and the barrier), and asserts
//   * every fragment read of a real K step sees the tile, group and stream step it is about to multiply, requested at least
//     FLIGHT + 1 passes earlier (the counted wait of pass W leaves the requests of W, W - 1, W - 2 in flight; a read in pass T
//     relies on the wait of T - 1);
//   * no piece and no ring slot is overwritten before its content has been read for the last time, and none is requested in the
//     pass of that last read;
//   * every pass's wait count is the number of requests of the last FLIGHT passes, across the window seam and the tile seam;
//   * every real step of every tile is read exactly once, the zero steps read zero tiles of the stream.
// It then packs input-permuted weight images with at most 96 live channels and asserts that the steps 75 .. 99 of the stream, which
// the three-group walk reads as its zero steps (75 .. 79), are zero.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "../../simple_image_compression_network_amd/csrc/conv_walk.hpp"

using namespace sicn;
using namespace sicn::xw;

static int failures = 0;
#define CHECK(cond, ...) \
    do { \
        if (!(cond)) { \
            std::printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__); \
            std::printf("\n"); \
            if (++failures > 20) std::exit(1); \
        } \
    } while (0)

struct Piece {
    int tile = -1, group = -1, requested = 0, reads = 0, last_read = -1000;
};
struct Slot {
    int tile = -1, step = -1, requested = 0, last_read = -1000;
    bool read = false;
};

static int plane_of_tap(int t)   // the parity plane of a tap, from the tap itself
{
    const Tap a = conv_tap(t);
    return (a.ky & 1) * 2 + (a.kx & 1);
}
static int taps_of_plane(int pl)
{
    int n = 0;
    for (int t = 0; t < 25; t++) n += plane_of_tap(t) == pl;
    return n;
}

static void replay(int NG)
{
    const int NP = conv_npass(NG), STEPS = 2 * NP, REAL = 25 * NG, TILES = 3;
    CHECK(NP == (NG == 3 ? 40 : 50), "NG %d", NG);
    CHECK(STEPS % RING == 0 && STEPS >= REAL, "NG %d", NG);
    Piece piece[4][5];
    Slot ring[RING];
    std::set<std::tuple<int, int>> seen;   // (tile, step) of the real steps that were read
    std::vector<int> issued;               // requests per global pass
    // the prologue of the first tile: planes 0, 1 and slots 0 .. 2 of plane 2 with group 0, the ring with steps 0 .. 9; all of it
    // has landed (vmcnt(0) + barrier) before anything is read
    const int LONG_AGO = -100;
    for (int pl = 0; pl < 3; pl++)
        for (int s = 0; s < (pl < 2 ? 5 : 3); s++) piece[pl][s] = Piece{0, 0, LONG_AGO, 0, -1000};
    for (int s = 0; s < RING; s++) ring[s] = Slot{0, s, LONG_AGO, -1000, false};

    auto read_step = [&](int tile, int step, int G) {   // one K half of a fragment read in global pass G
        Slot &r = ring[step % RING];
        CHECK(r.tile == tile && r.step == step, "NG %d pass %d: ring slot %d holds (tile %d, step %d), wanted (%d, %d)", NG, G, step % RING,
              r.tile, r.step, tile, step);
        CHECK(r.requested <= G - (FLIGHT + 1), "NG %d pass %d: step %d was requested in pass %d", NG, G, step, r.requested);
        CHECK(!r.read, "NG %d pass %d: step %d read twice", NG, G, step);
        r.read = true;
        r.last_read = G;
        if (step >= REAL) return;   // a zero step: whatever the planes hold, times the zero tile that was just checked to be there
        const int group = step / 25, tap = step - 25 * group, pl = plane_of_tap(tap);
        for (int s = 0; s < 5; s++) {   // the four waves' fragments of a tap cover the whole plane
            Piece &p = piece[pl][s];
            CHECK(p.tile == tile && p.group == group, "NG %d pass %d step %d: plane %d slot %d holds (tile %d, group %d), wanted (%d, %d)", NG, G,
                  step, pl, s, p.tile, p.group, tile, group);
            CHECK(p.requested <= G - (FLIGHT + 1), "NG %d pass %d step %d: plane %d slot %d was requested in pass %d", NG, G, step, pl, s,
                  p.requested);
            p.reads++;
            p.last_read = G;
        }
        CHECK(seen.insert({tile, step}).second, "NG %d: (tile %d, step %d) read twice", NG, tile, step);
    };

    // the fragments of pass 0 of the first tile are read behind the prologue
    read_step(0, 0, -1);
    read_step(0, 1, -1);
    for (int n = 0; n < TILES; n++)
        for (int T = 0; T < NP; T++) {
            const int G = n * NP + T;
            // ---- the reads of the next pass's fragments
            const int tn = n + (T == NP - 1 ? 1 : 0);
            for (int half = 0; half < 2; half++) {
                const int step = conv_read_step(NG, T, half);
                CHECK(step == (2 * (T + 1) + half) % STEPS, "NG %d T %d", NG, T);
                if (tn < TILES) read_step(tn, step, G);
            }
            // ---- this pass's requests; what they overwrite must have been read for the last time in an earlier pass
            int count = 0;
            for (int idx = 0; idx < 2; idx++) {
                const int ahead = 2 * T + RING + idx, step = conv_ring_step(NG, T, idx), slot = conv_ring_slot(T, idx);
                CHECK(step == ahead % STEPS && slot == step % RING, "NG %d T %d", NG, T);
                Slot &r = ring[slot];
                CHECK(r.read && r.last_read < G, "NG %d pass %d: ring slot %d (tile %d, step %d) overwritten before its read", NG, G, slot, r.tile,
                      r.step);
                r = Slot{n + ahead / STEPS, step, G, -1000, false};
                count++;
            }
            for (int idx = 0; idx < 2; idx++) {
                const Refresh f = conv_refresh(NG, T, idx);
                if (f.plane < 0) continue;
                CHECK(f.plane < 4 && f.slot >= 0 && f.slot < 5, "NG %d T %d", NG, T);
                // the kernel requests with the offsets of the tile it is on until conv_switch_pass, of the next tile from there
                const int tile = n + (T >= conv_switch_pass(NG) ? 1 : 0), group = conv_piece_group(NG, T, f.kind);
                Piece &p = piece[f.plane][f.slot];
                if (p.tile >= 0) {
                    CHECK(p.reads == taps_of_plane(f.plane), "NG %d pass %d: plane %d slot %d (tile %d, group %d) overwritten after %d of %d reads",
                          NG, G, f.plane, f.slot, p.tile, p.group, p.reads, taps_of_plane(f.plane));
                    CHECK(p.last_read < G, "NG %d pass %d: plane %d slot %d requested in the pass of its last read", NG, G, f.plane, f.slot);
                }
                CHECK(group >= 0 && group < NG, "NG %d T %d: group %d", NG, T, group);
                p = Piece{tile, group, G, 0, -1000};
                count++;
            }
            issued.push_back(count);
            CHECK(count == conv_requests(NG, T), "NG %d T %d", NG, T);
            // ---- the counted wait.  (The first tile's passes 0 and 1 count requests of a tile in front that did not run: the prologue
            // drained everything, so a count above what is in flight waits for nothing and lets nothing through uncounted.)
            if (G >= FLIGHT - 1) {
                int want = 0;
                for (int i = 0; i < FLIGHT; i++) want += issued[(size_t)(G - i)];
                CHECK(conv_in_flight(NG, T) == want, "NG %d pass %d: wait count %d, requests of the last %d passes %d", NG, G,
                      conv_in_flight(NG, T), FLIGHT, want);
            } else {
                int have = 0;
                for (int i = 0; i <= G; i++) have += issued[(size_t)i];
                CHECK(conv_in_flight(NG, T) >= have, "NG %d pass %d", NG, G);
            }
        }
    CHECK((int)seen.size() == TILES * REAL, "NG %d: %d real steps read, %d expected", NG, (int)seen.size(), TILES * REAL);
    std::printf("replay NG=%d: %d passes per tile, %d real steps read over %d tiles\n", NG, NP, (int)seen.size(), TILES);
}

// an input-permuted 128 -> 128 image with n_live live input channels: dense random weights on them, the live channels at the positions
// 0 .. n_live - 1 (what sicn_live.h's group_permutation does to layer 1's weights), packed by the packer the library uses
static void stream_tail(int n_live, unsigned seed)
{
    const int C = 128;
    std::vector<uint8_t> alive((size_t)C, 0);
    unsigned x = seed;
    auto rnd = [&]() { return x = x * 1664525u + 1013904223u, x >> 8; };
    for (int k = 0; k < n_live;) {
        const int c = (int)(rnd() % C);
        if (!alive[(size_t)c]) alive[(size_t)c] = 1, k++;
    }
    std::vector<int> p((size_t)C);
    int at = 0;
    for (int pass = 0; pass < 2; pass++)
        for (int c = 0; c < C; c++)
            if ((alive[(size_t)c] != 0) == (pass == 0)) p[(size_t)c] = at++;
    std::vector<int8_t> w((size_t)C * 25 * C, 0), wp(w.size(), 0);
    for (int o = 0; o < C; o++)
        for (int t = 0; t < 25; t++)
            for (int c = 0; c < C; c++)
                if (alive[(size_t)c]) w[((size_t)o * 25 + t) * C + c] = (int8_t)(1 + rnd() % 100);   // never zero
    for (int o = 0; o < C; o++)
        for (int t = 0; t < 25; t++)
            for (int c = 0; c < C; c++) wp[((size_t)o * 25 + t) * C + p[(size_t)c]] = w[((size_t)o * 25 + t) * C + c];
    const size_t tb = (size_t)C * 32;
    std::vector<int8_t> s(100 * tb, 1);
    pack_conv_stream16(wp.data(), C, C, s.data());
    for (int step = 0; step < 100; step++) {
        bool any = false;
        for (size_t b = 0; b < tb; b++) any |= s[(size_t)step * tb + b] != 0;
        const bool want = (step / 25) * 32 < n_live;   // a step of a group with a live position
        CHECK(any == want, "%d live: step %d is %s", n_live, step, any ? "non-zero" : "zero");
    }
    CHECK(conv_inputs_zero_from(wp.data(), C, C, 96) == (n_live <= 96), "%d live", n_live);
    CHECK(conv_inputs_zero_from(wp.data(), C, C, n_live), "%d live", n_live);
    if (n_live > 0) CHECK(!conv_inputs_zero_from(wp.data(), C, C, n_live - 1), "%d live", n_live);
    std::printf("stream %d live: steps %d .. 99 zero\n", n_live, 25 * ((n_live + 31) / 32));
}

int main()
{
    replay(4);
    replay(3);
    stream_tail(80, 1u);
    stream_tail(96, 2u);
    stream_tail(65, 3u);
    stream_tail(97, 4u);   // the control: a live channel in group 3, steps 75 .. 99 are not zero and the host's assertion says so
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("conv_walk_check ok\n");
    return 0;
}
