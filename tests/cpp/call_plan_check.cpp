// Stand-alone check of the live-channel plan and of the plan of one call (csrc/sicn_live.h), host C++ only: tests/test_live_plan.py and
// tests/test_l0_groups_plan.py compile this file with -fsanitize=address,undefined and run it on weight sets they write to a directory.
//   call_plan_check DIR N first last tap_layer
// DIR holds, per layer l = 0 .. N - 1, `l<l>.okc` (int8 [cout][25 cin]), `l<l>.bias` (int8 [cout]) and one line of `meta.txt`:
//   cin cout gdn wide link_layout transposed l7      (the last four: live::CallFacts, what the call knows of the layer; link_layout is
//                                                     the layout towards the next layer, 0 = NHWC, 1 = GROUP, 2 = PHASE)
// Output, per layer, what live::plan_call makes of it (`ng`: the table's groups; the rest is the layer's live::Step):
//   `L <l> live <n> nj <columns> ng <table> groups <out> groups_in <in> variant <2 in + out> halves <1 | 2> walk <3 | 4>`
// and its permutation, `P <l> p0 p1 ...` for a layer that skips columns in this call, `G <l> p0 p1 ...` for one that skips a group; the
// permuted copies are written next to the inputs: `l<l>.out.okc` / `l<l>.out.bias` (its own rows and bias moved) and `l<l+1>.in.okc`
// (the consumer's K index moved).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../simple_image_compression_network_amd/csrc/sicn_live.h"

using namespace sicn;

static std::vector<int8_t> slurp(const std::string &path, size_t want)
{
    std::ifstream f(path, std::ios::binary);
    std::vector<int8_t> v(want);
    if (!f.read((char *)v.data(), (std::streamsize)want) || f.peek() != EOF) {
        fprintf(stderr, "%s: not %zu bytes\n", path.c_str(), want);
        exit(2);
    }
    return v;
}
static void spill(const std::string &path, const std::vector<int8_t> &v)
{
    std::ofstream f(path, std::ios::binary);
    f.write((const char *)v.data(), (std::streamsize)v.size());
}

int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    const std::string dir = argv[1];
    const int n = atoi(argv[2]), first = atoi(argv[3]), last = atoi(argv[4]), tap = atoi(argv[5]);
    std::vector<live::Layer> L((size_t)n);
    std::vector<live::CallFacts> facts((size_t)n);
    std::vector<std::vector<int8_t>> okc((size_t)n), bias((size_t)n);
    std::ifstream meta(dir + "/meta.txt");
    for (int l = 0; l < n; l++) {
        live::Layer &y = L[(size_t)l];
        live::CallFacts &f = facts[(size_t)l];
        int gdn = 0, wide = 0, transposed = 0, l7 = 0;
        if (!(meta >> y.cin >> y.cout >> gdn >> wide >> f.link_layout >> transposed >> l7)) return 2;
        y.gdn = gdn != 0;
        f.wide = wide != 0;
        f.transposed = transposed != 0;
        f.l7 = l7 != 0;
        okc[(size_t)l] = slurp(dir + "/l" + std::to_string(l) + ".okc", (size_t)y.cout * 25 * y.cin);
        bias[(size_t)l] = slurp(dir + "/l" + std::to_string(l) + ".bias", (size_t)y.cout);
        y.in_mask = live::live_inputs(okc[(size_t)l].data(), y.cin, y.cout);
    }
    live::make_tables(L, false);
    std::vector<live::Step> steps((size_t)n);
    live::plan_call(L, facts.data(), n, first, last, tap, steps.data());
    for (int l = 0; l < n; l++) {
        const live::Step &s = steps[(size_t)l];
        printf("L %d live %d nj %d ng %d groups %d groups_in %d variant %d halves %d walk %d\n", l, s.live_out, s.cols, L[(size_t)l].ng, s.groups,
               s.groups_in, s.variant, s.halves, s.walk_groups);
        if (!live::wrote_permuted(s.cols, s.groups)) continue;
        const std::vector<int> &p = L[(size_t)l].p;
        printf("%s %d", s.cols < live::COLS ? "P" : "G", l);
        for (int v : p) printf(" %d", v);
        printf("\n");
        std::vector<int8_t> w(okc[(size_t)l].size()), b(bias[(size_t)l].size()), k(okc[(size_t)l + 1].size());
        live::permute_outputs(okc[(size_t)l].data(), bias[(size_t)l].data(), L[(size_t)l].cin, p, w.data(), b.data());
        live::permute_inputs(okc[(size_t)l + 1].data(), L[(size_t)l + 1].cout, p, k.data());
        spill(dir + "/l" + std::to_string(l) + ".out.okc", w);
        spill(dir + "/l" + std::to_string(l) + ".out.bias", b);
        spill(dir + "/l" + std::to_string(l + 1) + ".in.okc", k);
    }
    return 0;
}
