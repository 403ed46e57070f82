// The live-channel plan of a layer chain (host C++ only: no HIP, no device; tests/cpp/call_plan_check.cpp compiles it alone).
//
// A layer's output channel that its only consumer multiplies by zero in every tap need not be computed.  The wide persistent
// kernels (k_mfma16x.hip, k_mfma16x_live.hip) hold a 16 x 32-position tile as 8 accumulator COLUMNS of 16 channels; column
// j = 4 J + d holds the physical channel positions 64 J + 16 g + 4 d + r (g, r = 0 .. 3).  A layer that computes only NJ columns
// writes logical channel c at the physical position p(c):
//   * the live channels, in ascending order, go to the positions of columns 0 .. NJ - 1, in ascending order;
//   * the dead channels, in ascending order, go to the positions that remain (some may land in a computed column: harmless).
// The layer's own weight rows and bias are packed in that order, the consumer's K index is permuted by the same p: both are copies
// of w_okc ([cout][25 cin], k = tap cin + c) with rows or columns moved, which then go through the ordinary packers.  The bytes at
// positions nobody computes are undefined; they meet zero weights, and integer arithmetic makes that exact.
//
// A layer that is not a 128 -> 128 layer but whose 128 output channels leave in the GROUP layout ([n][C / 32][H][W][32]: the layer-0
// RGB family, cin = 3) has no columns to skip, but it can skip a whole 32-channel GROUP, which is a plane of the tensor: with at most
// 96 live channels it computes and stores NG = 3 groups, and p puts the live channels, ascending, at the positions 0, 1, 2, ... and the
// dead ones, ascending, behind them.  Plane 3 then holds dead channels only and stays what the workspace held.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace sicn {
namespace live {

constexpr int CH = 128;                      // channels of the wide family (128 -> 128)
constexpr int COLS = 8;                      // accumulator columns of 16 channels
constexpr int WIDTHS[] = {3, 5, 8};          // the column counts kernels are built for (8: k_mfma16x.hip, today's kernels)
constexpr int GROUPS = 4;                    // 32-channel groups = planes of the GROUP layout
constexpr int GROUP_CH = 32;

constexpr int column_of(int pos) { return 4 * (pos >> 6) + ((pos >> 2) & 3); }

// mask[c] = 1 where input channel c of w_okc [cout][25 cin] has a non-zero weight in any tap of any output row
inline std::vector<uint8_t> live_inputs(const int8_t *w_okc, int cin, int cout)
{
    std::vector<uint8_t> m((size_t)cin, 0);
    const size_t kk = (size_t)25 * cin;
    for (int o = 0; o < cout; o++)
        for (int t = 0; t < 25; t++) {
            const int8_t *src = w_okc + (size_t)o * kk + (size_t)t * cin;
            for (int c = 0; c < cin; c++) m[(size_t)c] |= (uint8_t)(src[c] != 0);
        }
    return m;
}

inline int count_live(const std::vector<uint8_t> &m)
{
    int n = 0;
    for (uint8_t v : m) n += v != 0;
    return n;
}

// live channels -> whole columns -> the next width that is built
inline int built_width(int n_live)
{
    const int cols = (n_live + 15) / 16;
    for (int w : WIDTHS)
        if (cols <= w) return w;
    return COLS;
}

// p[c] = physical position of logical channel c for a layer that computes columns 0 .. nj - 1 (mask: CH entries)
inline std::vector<int> permutation(const std::vector<uint8_t> &mask, int nj)
{
    std::vector<int> head, tail, p((size_t)CH, -1);
    for (int pos = 0; pos < CH; pos++) (column_of(pos) < nj ? head : tail).push_back(pos);
    head.insert(head.end(), tail.begin(), tail.end());   // computed positions first, each part ascending
    size_t at = 0;
    for (int pass = 0; pass < 2; pass++)
        for (int c = 0; c < CH; c++)
            if ((mask[(size_t)c] != 0) == (pass == 0)) p[(size_t)c] = head[at++];
    return p;
}

// a non-wide producer's group count: 3 where the live channels fit three planes, otherwise all 4 (only these two are built)
inline int built_groups(int n_live) { return n_live <= 3 * GROUP_CH ? 3 : GROUPS; }

// p[c] for a layer that writes whole groups: live channels ascending to 0, 1, 2, ..., dead channels ascending to the rest
inline std::vector<int> group_permutation(const std::vector<uint8_t> &mask)
{
    std::vector<int> p((size_t)CH, -1);
    int at = 0;
    for (int pass = 0; pass < 2; pass++)
        for (int c = 0; c < CH; c++)
            if ((mask[(size_t)c] != 0) == (pass == 0)) p[(size_t)c] = at++;
    return p;
}

// the producer's side: row p[c] of dst = row c of w_okc, bias likewise (cout = CH rows of 25 cin)
inline void permute_outputs(const int8_t *w_okc, const int8_t *bias, int cin, const std::vector<int> &p, int8_t *w_dst, int8_t *b_dst)
{
    const size_t kk = (size_t)25 * cin;
    for (int c = 0; c < CH; c++) {
        const int8_t *src = w_okc + (size_t)c * kk;
        int8_t *dst = w_dst + (size_t)p[(size_t)c] * kk;
        for (size_t k = 0; k < kk; k++) dst[k] = src[k];
        b_dst[p[(size_t)c]] = bias[c];
    }
}

// the consumer's side: dst[o][tap CH + p[c]] = w_okc[o][tap CH + c] (cin = CH)
inline void permute_inputs(const int8_t *w_okc, int cout, const std::vector<int> &p, int8_t *w_dst)
{
    const size_t kk = (size_t)25 * CH;
    for (int o = 0; o < cout; o++)
        for (int t = 0; t < 25; t++) {
            const int8_t *src = w_okc + (size_t)o * kk + (size_t)t * CH;
            int8_t *dst = w_dst + (size_t)o * kk + (size_t)t * CH;
            for (int c = 0; c < CH; c++) dst[p[(size_t)c]] = src[c];
        }
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------
// What is known of layer i when the net is made (Layer), and what one call makes of it (plan_call).
struct Layer {
    int cin = 0, cout = 0;
    bool gdn = false;             // carries a sicn_gdn: the activation mixes channels, every channel is needed
    std::vector<uint8_t> in_mask; // live_inputs of its own weights
    // made by make_tables():
    int live_out = 0;             // output channels the chain needs from it (cout: all)
    int nj = COLS;                // built width for them; COLS where the layer can never skip a column
    int ng = GROUPS;              // groups a non-wide producer of 128 channels computes; GROUPS where it can never skip one
    std::vector<int> p;           // nj < COLS or ng < GROUPS: where it writes its channels (empty: in their own order)
};

// creation: layer i + 1 is layer i's only consumer.  force_generic: no layer runs on the wide family.
inline void make_tables(std::vector<Layer> &L, bool force_generic)
{
    const size_t n = L.size();
    for (size_t i = 0; i < n; i++) {
        Layer &l = L[i];
        l.live_out = l.cout;
        l.nj = COLS;
        l.ng = GROUPS;
        l.p.clear();
        if (i + 1 < n && !l.gdn && (int)L[i + 1].in_mask.size() == l.cout) l.live_out = count_live(L[i + 1].in_mask);
        const bool wide_shape = l.cin == CH && l.cout == CH;
        if (wide_shape && !l.gdn && !force_generic && i + 1 < n) l.nj = built_width(l.live_out);
        if (l.nj < COLS) l.p = permutation(L[i + 1].in_mask, l.nj);
        const bool rgb_shape = l.cin == 3 && l.cout == CH;   // the layer-0 RGB family: 128 channels out in the GROUP layout
        if (rgb_shape && !l.gdn && !force_generic && i + 1 < n && (int)L[i + 1].in_mask.size() == l.cout) l.ng = built_groups(l.live_out);
        if (l.ng < GROUPS) l.p = group_permutation(L[i + 1].in_mask);
    }
}

// one call: the output channels of layer i that somebody reads (the last layer's and the tapped layer's leave the chain)
inline int live_outputs(const std::vector<Layer> &L, int i, int first, int last, int tap_layer)
{
    if (i < first || i >= last || i == tap_layer) return L[(size_t)i].cout;
    return L[(size_t)i].live_out;
}

// one call: the columns layer i computes.  wide: the layer is planned onto the wide family for this call (plan_mfma family 2).
inline int columns(const std::vector<Layer> &L, int i, int first, int last, int tap_layer, bool wide)
{
    if (i < first || i >= last || i == tap_layer || !wide) return COLS;
    return L[(size_t)i].nj;
}

// one call: the groups layer i computes and stores.  group_layout: its output leaves in the GROUP layout in this call.
inline int groups(const std::vector<Layer> &L, int i, int first, int last, int tap_layer, bool group_layout)
{
    if (i < first || i >= last || i == tap_layer || !group_layout) return GROUPS;
    return L[(size_t)i].ng;
}

// one call: a layer that skipped columns or a group wrote its channels in the order of its p, and which copy of a layer's weights a
// call takes follows from that on both sides: 2 (the layer in front of it in this call wrote permuted channels) + 1 (it does itself);
// 0 is the caller's own handle
inline bool wrote_permuted(int cols, int groups) { return cols < COLS || groups < GROUPS; }
inline int variant(int cols_in, int groups_in, int cols, int groups)
{
    return 2 * (int)wrote_permuted(cols_in, groups_in) + (int)wrote_permuted(cols, groups);
}

// Layer 7 reads only the first 64-channel half of its input where the layer in front of it, in this call, computed at most 4
// accumulator columns: column_of(pos) < 4 <=> pos < 64, so every live channel sits in the 32-channel groups 0 and 1,
// the weights of the groups 2 and 3 are zero in the permuted image this layer got, and (a layer with a GDN computes all 8) no
// activation has mixed the channels.  The GROUP and PHASE layouts keep a group in a plane of its own: the two planes that are skipped
// are whole; NHWC would leave half of every line unread for nothing.
inline int input_halves(bool l7, int cols_in, int in_layout) { return (l7 && cols_in <= 4 && in_layout != 0) ? 1 : 2; }

// The one rule of the three-group walk: a conv on the wide family whose input's producer computed and stored three groups in this call.
// Only a net's plan says groups_in == 3 (the per-layer entry points and the ragged nets say 4), and then the layer runs on the
// input-permuted copy of its weights (group_permutation puts every dead channel at a position >= 96), whose stream steps 75 .. 99 —
// group 3 — are all-zero tiles: make_live_plan asserts it.  k_conv_g3 reads that same d_w_mfma16 through a descriptor of 80 steps, the
// ring wrapping there: 75 real steps and the zero tiles 75 .. 79 (conv_walk.hpp).
inline int walk_groups(bool wide, bool transposed, int groups_in) { return (wide && !transposed && groups_in == 3) ? 3 : GROUPS; }

// ---- one call ---------------------------------------------------------------------------------------------------------------
// What the host layer knows of a layer for one call's options, image count and chip (csrc/sicn_abi.hip: call_facts).
struct CallFacts {
    bool wide = false;        // planned onto the wide family (plan_mfma family 2)
    bool transposed = false;
    bool l7 = false;          // runs on the layer-7 RGB family
    int link_layout = 0;      // the layout both this layer and the next one implement (0 for the net's last layer)
    bool deals = false;       // wants zeroed tile-deal words
};

// What one call does with a layer.  The default is "everything whole, NHWC": a layer outside [first, last], and a layer run alone.
struct Step {
    int in_layout = 0, out_layout = 0;
    int cols = COLS, cols_in = COLS;         // accumulator columns it computes / the layer that wrote its input computed
    int groups = GROUPS, groups_in = GROUPS; // 32-channel groups it computes and stores / the layer that wrote its input did
    int variant = 0;                         // the copy of its weights it takes
    int halves = 2;                          // 64-channel halves of its input it reads (input_halves)
    int walk_groups = GROUPS;                // groups of its input its K walk covers (walk_groups)
    int live_out = 0;                        // output channels somebody reads (plan_call: live_outputs, for every layer of the net)
};

// The walk over a call's layers, the only one: out[0 .. n_layers - 1]; the chain's input is NHWC, the last and the tapped layer leave
// in NHWC, intermediates nobody outside sees travel in the layout both neighbours implement.
inline void plan_call(const std::vector<Layer> &L, const CallFacts *facts, int n_layers, int first, int last, int tap_layer, Step *out)
{
    for (int l = 0; l < n_layers; l++) {
        out[l] = Step{};
        out[l].live_out = live_outputs(L, l, first, last, tap_layer);
    }
    // the columns and groups the previous layer of this call computed: fewer than all of either = it wrote its channels in the order of its p
    int cols_before = COLS, groups_before = GROUPS, cur_layout = 0;
    for (int l = first; l <= last; l++) {
        const CallFacts &f = facts[l];
        Step &s = out[l];
        s.in_layout = cur_layout;
        s.out_layout = (l < last && l != tap_layer) ? f.link_layout : 0;
        s.cols = columns(L, l, first, last, tap_layer, f.wide);
        s.groups = groups(L, l, first, last, tap_layer, s.out_layout == 1);
        s.cols_in = cols_before;
        s.groups_in = groups_before;
        s.variant = variant(s.cols_in, s.groups_in, s.cols, s.groups);
        s.halves = input_halves(f.l7, s.cols_in, s.in_layout);
        s.walk_groups = walk_groups(f.wide, f.transposed, s.groups_in);
        cols_before = s.cols;
        groups_before = s.groups;
        cur_layout = s.out_layout;
    }
}

}  // namespace live
}  // namespace sicn
