// The K walk of the wide persistent conv (k_mfma16x_body.hpp: conv_x_body) as plain constexpr C++: the tap order, the weight stream's
// step order, the ring slots and the plane refresh schedule, for a tile that walks all four 32-channel groups of its input (NG = 4) or
// the first three (NG = 3).  No HIP types: the kernels include this, and so does tests/cpp/conv_walk_check.cpp, which replays the
// schedule pass by pass on the host.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIP__
#define SICN_WALK_FN __host__ __device__
#else
#define SICN_WALK_FN
#endif

namespace sicn {

// ---- conv tap order: by parity plane (a,b) = (ky&1, kx&1), so that a plane's LDS buffer is
// ---- free for the next channel group as soon as its taps are done (k_mfma.hip) -------------
struct Tap { int ky, kx; };
SICN_WALK_FN constexpr Tap conv_tap(int t)
{
    int n = 0;
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++)
            for (int ky = a; ky < 5; ky += 2)
                for (int kx = b; kx < 5; kx += 2) {
                    if (n == t) return Tap{ky, kx};
                    n++;
                }
    return Tap{-1, -1};
}

// ---- host-side weight packing of the 16x16x64 kernels' conv stream: step q * 25 + t = (channel group q, tap conv_tap(t)), one tile
// ---- of cout rows x 32 bytes per step, rows in the 16x16 C/D order (row j*16 + rho holds channel 64*(j>>2) + 16*(rho>>2) + 4*(j&3)
// ---- + (rho&3)), no swizzle.  Group-major: the steps of groups 0 .. n - 1 are the first 25 n of the stream.
inline void pack_tile16(const int8_t *w_okc, int cin, int cout, int tap, int q, int8_t *tile)
{
    const int kk = 25 * cin;
    for (int row = 0; row < cout; row++) {
        const int j = row >> 4, rho = row & 15;
        const int ch = 64 * (j >> 2) + 16 * (rho >> 2) + 4 * (j & 3) + (rho & 3);
        const int8_t *src = w_okc + (size_t)ch * kk + tap * cin + q * 32;
        for (int b = 0; b < 32; b++) tile[row * 32 + b] = src[b];
    }
}
inline void pack_conv_stream16(const int8_t *w_okc, int cin, int cout, int8_t *dst)
{
    const size_t tb = (size_t)cout * 32;
    size_t step = 0;
    for (int q = 0; q < cin / 32; q++)
        for (int t = 0; t < 25; t++) {
            const Tap tap = conv_tap(t);
            pack_tile16(w_okc, cin, cout, tap.ky * 5 + tap.kx, q, dst + (step++) * tb);
        }
}
// the three-group walk's invariant: it reads the steps 75 .. 79 of a four-group stream as its zero steps, so the weight image must
// have no non-zero weight on an input channel at position 96 or above (sicn_live.h: group_permutation puts every dead channel there)
inline bool conv_inputs_zero_from(const int8_t *w_okc, int cin, int cout, int from)
{
    for (int o = 0; o < cout; o++)
        for (int t = 0; t < 25; t++)
            for (int c = from; c < cin; c++)
                if (w_okc[((size_t)o * 25 + t) * cin + c] != 0) return false;
    return true;
}

namespace xw {

constexpr int RING = 10;     // weight-ring slots: one K step of 128 output channels each
constexpr int FLIGHT = 3;    // passes whose requests may be in flight at a barrier

// the plane a tap reads (conv_tap's order: 9 / 6 / 6 / 4 taps of planes 0 .. 3) and each plane's first and last tap
SICN_WALK_FN constexpr int tap_plane(int t) { return t < 9 ? 0 : t < 15 ? 1 : t < 21 ? 2 : 3; }
SICN_WALK_FN constexpr int plane_first_tap(int pl) { return pl == 0 ? 0 : pl == 1 ? 9 : pl == 2 ? 15 : 21; }
SICN_WALK_FN constexpr int plane_last_tap(int pl) { return pl == 0 ? 8 : pl == 1 ? 14 : pl == 2 ? 20 : 24; }
SICN_WALK_FN constexpr bool tap_planes_ok()
{
    for (int t = 0; t < 25; t++) {
        const Tap a = conv_tap(t);
        if ((a.ky & 1) * 2 + (a.kx & 1) != tap_plane(t)) return false;
        if (t < plane_first_tap(tap_plane(t)) || t > plane_last_tap(tap_plane(t))) return false;
    }
    return true;
}
static_assert(tap_planes_ok(), "tap_plane follows conv_tap");

// The DMA schedule: one 25-pass window = two channel groups (50 K steps); a four-group tile is two windows.  Plane pl of the group the
// window starts with is last READ (fragments are fetched one pass ahead of their MFMAs) in pass 3 / 6 / 9 / 11, of the window's
// second group in pass 15 / 18 / 21 / 23; it is re-filled from the pass after that.  What a pass reads was requested at least
// FLIGHT + 1 passes earlier.  KIND: which group a piece belongs to —
//   CUR0: the window's first group (the tail of plane 2 and plane 3, requested in the window's first passes)
//   CUR1: the window's second group
//   NEXT0: the first group of the NEXT window (in a tile's last window: of the workgroup's next tile)
enum { K_CUR0 = 0, K_CUR1 = 1, K_NEXT0 = 2 };
struct Refresh {
    int plane, slot, kind;
};
SICN_WALK_FN constexpr Refresh refresh_x(int P, int idx)   // the idx-th (0 / 1) piece of window pass P, plane < 0: none
{
    constexpr Refresh none{-1, 0, 0};
    switch (P) {
    case 0: return idx == 0 ? Refresh{2, 3, K_CUR0} : Refresh{3, 0, K_CUR0};
    case 1: return idx == 0 ? Refresh{2, 4, K_CUR0} : Refresh{3, 1, K_CUR0};
    case 2: return idx == 0 ? Refresh{3, 2, K_CUR0} : none;
    case 3: return idx == 0 ? Refresh{3, 3, K_CUR0} : none;
    case 4: return idx == 0 ? Refresh{3, 4, K_CUR0} : Refresh{0, 0, K_CUR1};
    case 5: return idx == 0 ? Refresh{0, 1, K_CUR1} : none;
    case 6: return idx == 0 ? Refresh{0, 2, K_CUR1} : Refresh{0, 3, K_CUR1};
    case 7: return idx == 0 ? Refresh{0, 4, K_CUR1} : Refresh{1, 0, K_CUR1};
    case 8: return idx == 0 ? Refresh{1, 1, K_CUR1} : none;
    case 9: return idx == 0 ? Refresh{1, 2, K_CUR1} : none;
    case 10: return idx == 0 ? Refresh{1, 3, K_CUR1} : Refresh{2, 0, K_CUR1};
    case 11: return idx == 0 ? Refresh{1, 4, K_CUR1} : Refresh{2, 1, K_CUR1};
    case 12: return idx == 0 ? Refresh{2, 2, K_CUR1} : Refresh{3, 0, K_CUR1};
    case 13: return idx == 0 ? Refresh{2, 3, K_CUR1} : Refresh{3, 1, K_CUR1};
    case 14: return idx == 0 ? Refresh{2, 4, K_CUR1} : Refresh{3, 2, K_CUR1};
    case 15: return idx == 0 ? Refresh{3, 3, K_CUR1} : Refresh{3, 4, K_CUR1};
    case 16: return idx == 0 ? Refresh{0, 0, K_NEXT0} : none;
    case 17: return idx == 0 ? Refresh{0, 1, K_NEXT0} : none;
    case 18: return idx == 0 ? Refresh{0, 2, K_NEXT0} : none;
    case 19: return idx == 0 ? Refresh{0, 3, K_NEXT0} : Refresh{1, 0, K_NEXT0};
    case 20: return idx == 0 ? Refresh{0, 4, K_NEXT0} : Refresh{1, 1, K_NEXT0};
    case 21: return idx == 0 ? Refresh{1, 2, K_NEXT0} : none;
    case 22: return idx == 0 ? Refresh{1, 3, K_NEXT0} : Refresh{2, 0, K_NEXT0};
    case 23: return idx == 0 ? Refresh{1, 4, K_NEXT0} : Refresh{2, 1, K_NEXT0};
    case 24: return idx == 0 ? Refresh{2, 2, K_NEXT0} : none;
    }
    return none;
}
SICN_WALK_FN constexpr int requests_x(int P)   // LDS-DMA instructions a wave issues in window pass P (any integer P)
{
    const int p = ((P % 25) + 25) % 25;
    return 2 + (refresh_x(p, 0).plane >= 0) + (refresh_x(p, 1).plane >= 0);
}
SICN_WALK_FN constexpr int in_flight_x(int P)   // requests of the last FLIGHT passes
{
    int s = 0;
    for (int i = 0; i < FLIGHT; i++) s += requests_x(P - i);
    return s;
}
// MFMAs of window step s run in pass floor(s / 2) and their fragments are read one pass earlier
SICN_WALK_FN constexpr int step_read_pass(int s) { return (s >= 0 ? s / 2 : -((-s + 1) / 2)) - 1; }
// the schedule against the walk, checked at compile time: a piece of plane pl, kind k, requested in pass P must be requested
// after the plane's last read and FLIGHT + 1 passes before its first read
SICN_WALK_FN constexpr bool schedule_ok()
{
    int count[3][4] = {};
    for (int P = 0; P < 25; P++)
        for (int i = 0; i < 2; i++) {
            const Refresh r = refresh_x(P, i);
            if (r.plane < 0) continue;
            count[r.kind][r.plane] |= 1 << r.slot;
            // steps (window-local) at which the OLD content of the plane is last used and the NEW content first used
            int last_use_step = 0, first_use_step = 0;   // relative to this window's step 0
            if (r.kind == K_CUR0) { last_use_step = plane_last_tap(r.plane) - 25; first_use_step = plane_first_tap(r.plane); }
            else if (r.kind == K_CUR1) { last_use_step = plane_last_tap(r.plane); first_use_step = 25 + plane_first_tap(r.plane); }
            else { last_use_step = 25 + plane_last_tap(r.plane); first_use_step = 50 + plane_first_tap(r.plane); }
            const int last_read = step_read_pass(last_use_step), first_read = step_read_pass(first_use_step);
            if (P <= last_read) return false;               // would overwrite fragments still to be read
            if (P > first_read - 1 - FLIGHT) return false;   // would not be covered by the counted wait before its first read
        }
    // every plane's 5 slots exactly once per group: CUR0 carries plane 2 slots 3, 4 and plane 3; NEXT0 the rest
    for (int pl = 0; pl < 4; pl++) {
        if (count[K_CUR1][pl] != 31) return false;
        if ((count[K_CUR0][pl] | count[K_NEXT0][pl]) != 31 || (count[K_CUR0][pl] & count[K_NEXT0][pl]) != 0) return false;
    }
    return true;
}
static_assert(schedule_ok(), "conv refresh schedule violates the read / landing windows");

// ---- the three-group tile -----------------------------------------------------------------------------------------------------
// Where the layer in front computed and stored only the groups 0, 1, 2 (sicn_live.h) a tile is 80 K steps = 40 passes: the 75 real
// steps of the three groups and 5 zero steps, which keep the tile a multiple of 5 passes, so that every ring slot (RING = 10 steps)
// and LDS offset of the unrolled tile stays a compile-time constant.  The zero steps read the steps 75 .. 79 of the four-group stream
// (all-zero tiles: conv_inputs_zero_from) against taps 0 .. 4 of whatever plane 0 holds, which is a refill in progress: any bytes
// times zero weights, exact in integers — the argument the four-group walk uses for a plane nobody wrote.
//   window 0 (tile passes 0 .. 24): refresh_x as it is; its CUR1 is group 1, its NEXT0 pieces fetch group 2
//   window 1 (tile passes 25 .. 39, window passes 0 .. 14): refresh3_x —
//     CUR0: group 2's plane 2 slots 3, 4 and plane 3 in its passes 0 .. 4, as refresh_x has them; there is no CUR1
//     NEXT0: the 13 pieces of the NEXT TILE's group 0, from window pass 5 on (the tile switch, conv_switch_pass):
//       plane 0 is last read in window pass 3 and first read again in 14 (for the next tile's pass 0): requests in 4 .. 10
//       plane 1: last read in 6, first in 18: requests in 7 .. 14 (the window's last pass)
//       plane 2 slots 0 .. 2: last read in 9, first in 21: requests in 10 .. 14
constexpr int WIN1_PASSES = 15, WIN1_STEPS = 2 * WIN1_PASSES;
SICN_WALK_FN constexpr Refresh refresh3_x(int P, int idx)
{
    constexpr Refresh none{-1, 0, 0};
    switch (P) {
    case 0: return idx == 0 ? Refresh{2, 3, K_CUR0} : Refresh{3, 0, K_CUR0};
    case 1: return idx == 0 ? Refresh{2, 4, K_CUR0} : Refresh{3, 1, K_CUR0};
    case 2: return idx == 0 ? Refresh{3, 2, K_CUR0} : none;
    case 3: return idx == 0 ? Refresh{3, 3, K_CUR0} : none;
    case 4: return idx == 0 ? Refresh{3, 4, K_CUR0} : none;
    case 5: return idx == 0 ? Refresh{0, 0, K_NEXT0} : Refresh{0, 1, K_NEXT0};
    case 6: return idx == 0 ? Refresh{0, 2, K_NEXT0} : none;
    case 7: return idx == 0 ? Refresh{0, 3, K_NEXT0} : Refresh{1, 0, K_NEXT0};
    case 8: return idx == 0 ? Refresh{0, 4, K_NEXT0} : none;
    case 9: return idx == 0 ? Refresh{1, 1, K_NEXT0} : none;
    case 10: return idx == 0 ? Refresh{1, 2, K_NEXT0} : Refresh{2, 0, K_NEXT0};
    case 11: return idx == 0 ? Refresh{1, 3, K_NEXT0} : none;
    case 12: return idx == 0 ? Refresh{1, 4, K_NEXT0} : Refresh{2, 1, K_NEXT0};
    case 13: return idx == 0 ? Refresh{2, 2, K_NEXT0} : none;
    }
    return none;
}

// ---- one tile of NG groups, by tile pass T --------------------------------------------------------------------------------------
SICN_WALK_FN constexpr int conv_npass(int NG) { return NG == 3 ? 25 + WIN1_PASSES : 50; }   // passes (of two K steps) per tile
SICN_WALK_FN constexpr int conv_real_steps(int NG) { return 25 * NG; }                      // the steps behind them are zero steps
// from this pass of a tile on, every plane request belongs to the workgroup's next tile
SICN_WALK_FN constexpr int conv_switch_pass(int NG) { return NG == 3 ? 25 + 5 : 25 + 16; }
SICN_WALK_FN constexpr Refresh conv_refresh(int NG, int T, int idx)   // the idx-th plane piece of tile pass T (0 .. conv_npass - 1)
{
    if (NG == 3) return T < 25 ? refresh_x(T, idx) : refresh3_x(T - 25, idx);
    return refresh_x(T % 25, idx);
}
// the channel group a piece of `kind` requested in tile pass T carries (NEXT0 of the last window: group 0 of the next tile)
SICN_WALK_FN constexpr int conv_piece_group(int NG, int T, int kind)
{
    if (NG == 3) return T < 25 ? kind : (kind == K_CUR0 ? 2 : 0);
    const int win = T / 25;
    return kind == K_CUR0 ? 2 * win : kind == K_CUR1 ? 2 * win + 1 : (2 * win + 2) % 4;
}
SICN_WALK_FN constexpr int conv_requests(int NG, int T)   // LDS-DMA instructions a wave issues in tile pass T (any integer T: tiles repeat)
{
    const int np = conv_npass(NG), t = ((T % np) + np) % np;
    return 2 + (conv_refresh(NG, t, 0).plane >= 0) + (conv_refresh(NG, t, 1).plane >= 0);
}
SICN_WALK_FN constexpr int conv_in_flight(int NG, int T)   // requests of the last FLIGHT passes: the counted wait of tile pass T
{
    int s = 0;
    for (int i = 0; i < FLIGHT; i++) s += conv_requests(NG, T - i);
    return s;
}
// pass T reads the fragments of pass T + 1 (wrapping into the next tile): the tile step of K half `half`, its tap and its ring slot
SICN_WALK_FN constexpr int conv_read_step(int NG, int T, int half) { return 2 * ((T + 1) % conv_npass(NG)) + half; }
SICN_WALK_FN constexpr int conv_step_tap(int s) { return s % 25; }
SICN_WALK_FN constexpr int conv_step_group(int s) { return s / 25; }
SICN_WALK_FN constexpr int ring_slot(int s) { return s % RING; }
// pass T requests two weight tiles a whole ring ahead: the stream step (wrapping at the tile) of request idx (0 / 1); it goes to the slot
// of the step the pass's own MFMAs consume
SICN_WALK_FN constexpr int conv_ring_step(int NG, int T, int idx) { return (2 * T + RING + idx) % (2 * conv_npass(NG)); }
SICN_WALK_FN constexpr int conv_ring_slot(int T, int idx) { return ring_slot(2 * T + idx); }

SICN_WALK_FN constexpr bool walk4_is_the_window_walk()   // NG = 4: the tile-pass forms are the window forms the kernel had
{
    for (int T = 0; T < 50; T++) {
        if (conv_in_flight(4, T) != in_flight_x(T % 25)) return false;
        for (int i = 0; i < 2; i++) {
            const Refresh a = conv_refresh(4, T, i), b = refresh_x(T % 25, i);
            if (a.plane != b.plane || a.slot != b.slot || a.kind != b.kind) return false;
        }
    }
    return (2 * conv_npass(4)) % RING == 0;
}
static_assert(walk4_is_the_window_walk(), "the four-group walk");

// the three-group schedule against the walk, as schedule_ok() does it for the windows of the four-group one
SICN_WALK_FN constexpr bool schedule3_ok()
{
    if ((2 * conv_npass(3)) % RING != 0 || 2 * conv_npass(3) < conv_real_steps(3)) return false;
    int count[3][4] = {};
    for (int P = 0; P < WIN1_PASSES; P++)
        for (int i = 0; i < 2; i++) {
            const Refresh r = refresh3_x(P, i);
            if (r.plane < 0) continue;
            if (count[r.kind][r.plane] & (1 << r.slot)) return false;
            count[r.kind][r.plane] |= 1 << r.slot;
            int last_use_step = 0, first_use_step = 0;   // relative to this window's step 0 = tile step 50
            if (r.kind == K_CUR0) {            // over group 1's, for group 2
                last_use_step = plane_last_tap(r.plane) - 25;
                first_use_step = plane_first_tap(r.plane);
                if (25 + P >= conv_switch_pass(3)) return false;   // requested with this tile's offsets
            } else if (r.kind == K_NEXT0) {    // over group 2's, for the next tile's group 0, WIN1_STEPS on
                last_use_step = plane_last_tap(r.plane);
                first_use_step = WIN1_STEPS + plane_first_tap(r.plane);
                if (25 + P < conv_switch_pass(3)) return false;    // requested with the next tile's offsets
            } else {
                return false;
            }
            const int last_read = step_read_pass(last_use_step), first_read = step_read_pass(first_use_step);
            if (P <= last_read) return false;
            if (P > first_read - 1 - FLIGHT) return false;
        }
    // window 1 brings exactly what window 0 leaves open of group 2 (its NEXT0 set's complement) and what the next tile's window 0
    // expects to find of group 0 (the complement of its CUR0 set)
    int c0[4] = {}, n0[4] = {};
    for (int P = 0; P < 25; P++)
        for (int i = 0; i < 2; i++) {
            const Refresh r = refresh_x(P, i);
            if (r.plane < 0) continue;
            if (r.kind == K_CUR0) c0[r.plane] |= 1 << r.slot;
            if (r.kind == K_NEXT0) n0[r.plane] |= 1 << r.slot;
        }
    for (int pl = 0; pl < 4; pl++) {
        if (count[K_CUR0][pl] != (31 & ~n0[pl])) return false;
        if (count[K_NEXT0][pl] != (31 & ~c0[pl])) return false;
    }
    // a zero step reads plane 0 only, so no piece of another plane has to mind it
    for (int s = conv_real_steps(3); s < 2 * conv_npass(3); s++)
        if (tap_plane(conv_step_tap(s)) != 0 || conv_step_group(s) != 3) return false;
    return true;
}
static_assert(schedule3_ok(), "the three-group conv refresh schedule violates the read / landing windows");

}  // namespace xw
}  // namespace sicn
