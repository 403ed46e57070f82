// Stand-alone check of the channel groups of a non-wide producer in the live-channel plan (csrc/sicn_live.h), host C++ only:
// tests/test_l0_groups_plan.py compiles this file with -fsanitize=address,undefined and runs it on weight sets it writes to a directory.
//   l0_groups_plan_check DIR N first last tap_layer
// DIR holds, per layer l = 0 .. N - 1, `l<l>.okc` (int8 [cout][25 cin]), `l<l>.bias` (int8 [cout]) and one line of `meta.txt`:
//   cin cout gdn wide group      (wide: the call runs the layer on the wide family; group: its output leaves in the GROUP layout
//                                 where it is neither the call's last nor its tapped layer)
// Output, per layer, the walk of one call as sicn_net_forward makes it:
//   `L <l> live <n> nj <columns> ng <table> groups <out> groups_in <in> variant <2 in + out>`
// and for a layer whose table has ng < 4 its permutation (`P <l> p0 p1 ...`); the permuted copies are written next to the inputs:
// `l<l>.out.okc` / `l<l>.out.bias` (its own rows and bias moved) and `l<l+1>.in.okc` (the consumer's K index moved).
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
    std::vector<std::vector<int8_t>> okc((size_t)n), bias((size_t)n);
    std::vector<int> wide((size_t)n), group((size_t)n);
    std::ifstream meta(dir + "/meta.txt");
    for (int l = 0; l < n; l++) {
        int gdn = 0;
        if (!(meta >> L[(size_t)l].cin >> L[(size_t)l].cout >> gdn >> wide[(size_t)l] >> group[(size_t)l])) return 2;
        L[(size_t)l].gdn = gdn != 0;
        okc[(size_t)l] = slurp(dir + "/l" + std::to_string(l) + ".okc", (size_t)L[(size_t)l].cout * 25 * L[(size_t)l].cin);
        bias[(size_t)l] = slurp(dir + "/l" + std::to_string(l) + ".bias", (size_t)L[(size_t)l].cout);
        L[(size_t)l].in_mask = live::live_inputs(okc[(size_t)l].data(), L[(size_t)l].cin, L[(size_t)l].cout);
    }
    live::make_tables(L, false);
    int cols_before = live::COLS, groups_before = live::GROUPS;
    for (int l = 0; l < n; l++) {
        const bool in_call = l >= first && l <= last;
        const int nj = live::columns(L, l, first, last, tap, wide[(size_t)l] != 0);
        const int ng = live::groups(L, l, first, last, tap, group[(size_t)l] != 0);
        const int cols_in = in_call ? cols_before : live::COLS, groups_in = in_call ? groups_before : live::GROUPS;
        printf("L %d live %d nj %d ng %d groups %d groups_in %d variant %d\n", l, live::live_outputs(L, l, first, last, tap), nj, L[(size_t)l].ng,
               ng, groups_in, in_call ? live::variant(cols_in, groups_in, nj, ng) : 0);
        if (in_call) {
            cols_before = nj;
            groups_before = ng;
        }
        if (L[(size_t)l].ng >= live::GROUPS) continue;
        const std::vector<int> &p = L[(size_t)l].p;
        printf("P %d", l);
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
