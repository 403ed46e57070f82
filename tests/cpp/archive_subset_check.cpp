// Stand-alone check of sicn_archive::subset (csrc/archive_host.hpp: the archive of a selection of an archive's images) for builds
// with the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all archive_subset_check.cpp -o archive_subset_check
// Every source archive and every output lives in a heap block of EXACTLY its length, so a read or a write past either end is an
// AddressSanitizer report, not luck.  Exit status 0 and one line "archive_subset_check ok: <n> checks" when everything held.  No
// device, no library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../simple_image_compression_network_amd/csrc/archive_host.hpp"

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

using Bytes = std::vector<uint8_t>;

void put32(Bytes &b, size_t at, uint32_t v)
{
    for (int i = 0; i < 4; i++) b[at + i] = (uint8_t)(v >> (8 * i));
}

// the format, written down once more: containers[image * k + section] -> header, index, zero-padded containers
Bytes make(const std::vector<Bytes> &containers, uint32_t n, uint32_t k, uint32_t tag)
{
    size_t at = 32 + (4 * containers.size() + 15) / 16 * 16;
    std::vector<size_t> off;
    for (const Bytes &c : containers) {
        off.push_back(at);
        at += (c.size() + 15) / 16 * 16;
    }
    Bytes b(at, 0);
    std::memcpy(b.data(), "SICA", 4);
    b[4] = 1;
    b[6] = (uint8_t)k;
    put32(b, 8, n);
    put32(b, 12, tag);
    put32(b, 16, (uint32_t)at);
    put32(b, 20, (uint32_t)((uint64_t)at >> 32));
    for (size_t e = 0; e < containers.size(); e++) {
        put32(b, 32 + 4 * e, (uint32_t)containers[e].size());
        if (!containers[e].empty()) std::memcpy(b.data() + off[e], containers[e].data(), containers[e].size());
    }
    return b;
}

std::vector<Bytes> pattern(const std::vector<uint32_t> &sizes)
{
    std::vector<Bytes> out;
    for (size_t e = 0; e < sizes.size(); e++) {
        Bytes c(sizes[e]);
        for (uint32_t i = 0; i < sizes[e]; i++) c[i] = (uint8_t)(1 + (e * 7 + i) % 255);
        out.push_back(c);
    }
    return out;
}

// subset of the first `len` bytes of `b`, source and selection in heap blocks of exactly their lengths, the output in one of
// exactly `capacity` bytes (none when capacity < 0: out == NULL); *got: what was written
int subset_exact(const Bytes &b, size_t len, const std::vector<uint32_t> &sel, long capacity, Bytes *got, uint64_t *need)
{
    std::unique_ptr<uint8_t[]> src(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(src.get(), b.data(), len);
    std::unique_ptr<uint32_t[]> index(new uint32_t[sel.size() ? sel.size() : 1]);
    for (size_t j = 0; j < sel.size(); j++) index[j] = sel[j];
    if (capacity < 0) return sicn_archive::subset(src.get(), len, index.get(), (uint32_t)sel.size(), nullptr, 0, need);
    std::unique_ptr<uint8_t[]> out(new uint8_t[capacity ? capacity : 1]);
    std::memset(out.get(), 0xEE, capacity ? capacity : 1);
    const int rc = sicn_archive::subset(src.get(), len, index.get(), (uint32_t)sel.size(), out.get(), (size_t)capacity, need);
    if (got) got->assign(out.get(), out.get() + capacity);
    return rc;
}

void check_selection(const std::vector<uint32_t> &sizes, uint32_t n, uint32_t k, const std::vector<uint32_t> &sel)
{
    const std::vector<Bytes> containers = pattern(sizes);
    const Bytes src = make(containers, n, k, 0xC0FFEE02u);
    std::vector<Bytes> chosen;
    for (uint32_t i : sel)
        for (uint32_t s = 0; s < k; s++) chosen.push_back(containers[(size_t)i * k + s]);
    const Bytes want = make(chosen, (uint32_t)sel.size(), k, 0xC0FFEE02u);
    uint64_t need = 0;
    EXPECT(subset_exact(src, src.size(), sel, -1, nullptr, &need) == SICN_OK && need == want.size());
    Bytes got;
    need = 0;
    EXPECT(subset_exact(src, src.size(), sel, (long)want.size(), &got, &need) == SICN_OK && need == want.size());
    EXPECT(got == want);
    // the result is an archive, and of those containers
    sicn_ragged_archive_info info;
    std::vector<uint32_t> got_sizes(chosen.size());
    std::vector<uint64_t> got_off(chosen.size());
    EXPECT(sicn_archive::parse(got.data(), got.size(), &info, got_sizes.data(), got_off.data()) == SICN_OK);
    EXPECT(info.n_images == sel.size() && info.n_sections == k && info.tag == 0xC0FFEE02u && info.total_bytes == want.size());
    for (size_t e = 0; e < chosen.size(); e++)
        EXPECT(got_sizes[e] == chosen[e].size() && (chosen[e].empty() || std::memcmp(got.data() + got_off[e], chosen[e].data(), chosen[e].size()) == 0));
    // one byte short: SICN_ENOSPC, the size needed, nothing written
    if (!want.empty()) {
        need = 0;
        EXPECT(subset_exact(src, src.size(), sel, (long)want.size() - 1, &got, &need) == SICN_ENOSPC && need == want.size());
        bool untouched = true;
        for (uint8_t v : got) untouched &= v == 0xEE;
        EXPECT(untouched);
    }
    EXPECT(subset_exact(src, src.size(), sel, 0, &got, &need) == SICN_ENOSPC && need == want.size());
    // bytes behind the source's end are none of its business; a source cut anywhere is refused and nothing behind the cut is read
    Bytes longer = src;
    longer.resize(src.size() + 37, 0xAB);
    EXPECT(subset_exact(longer, longer.size(), sel, (long)want.size(), &got, &need) == SICN_OK && got == want);
    for (size_t len = 0; len < src.size(); len += (src.size() > 4096 ? 97 : 1))
        EXPECT(subset_exact(src, len, sel, (long)want.size(), &got, &need) == SICN_EINVAL && need == 0);
}

void check_hostile()
{
    const std::vector<uint32_t> sizes = {17, 40, 0, 16, 1, 33, 5, 0};            // 8 entries: an index without padding
    const uint32_t n = 4, k = 2;
    const Bytes good = make(pattern(sizes), n, k, 7);
    Bytes got;
    uint64_t need = 0;
    EXPECT(subset_exact(good, good.size(), {1, 3}, 4096, &got, &need) == SICN_OK);
    struct Patch { size_t at; uint32_t value; int bytes; };
    const Patch patches[] = {
        {0, 0x42434953u, 4}, {3, 'a', 1},                       // magic
        {4, 0, 2}, {4, 2, 2},                                   // version
        {24, 1, 4}, {28, 0x80000000u, 4},                       // reserved
        {6, 0, 2}, {6, 5, 2}, {6, 1, 2}, {6, 3, 2},             // n_sections
        {8, 0, 4}, {8, n + 1, 4}, {8, n - 1, 4}, {8, 0xFFFFFFFFu, 4}, {8, 1u << 24, 4},   // n_images
        {32 + 4, 0xFFFFFFF0u, 4}, {32 + 4, 40 + 16, 4}, {32 + 4, 0, 4}, {32 + 28, 16, 4},   // sizes, selected or not
        {16, (uint32_t)good.size() + 16, 4}, {16, (uint32_t)good.size() - 16, 4}, {16, (uint32_t)good.size() - 8, 4},   // total_bytes
        {20, 1, 4}, {16, 32, 4}, {16, 0, 4},
    };
    for (const Patch &p : patches) {
        Bytes b = good;
        for (int i = 0; i < p.bytes; i++) b[p.at + i] = (uint8_t)(p.value >> (8 * i));
        EXPECT(b != good);
        need = 77;
        EXPECT(subset_exact(b, b.size(), {1, 3}, 4096, &got, &need) == SICN_EINVAL && need == 0);
        bool untouched = true;
        for (uint8_t v : got) untouched &= v == 0xEE;
        EXPECT(untouched);
    }
    // the selection: an index == n_images, equal neighbours, descending, none
    const std::vector<std::vector<uint32_t>> bad = {{n}, {0, n}, {0xFFFFFFFFu}, {1, 1}, {0, 2, 2}, {2, 1}, {0, 3, 1}, {}, {0, 1, 2, 3, 3}};
    for (const auto &sel : bad) {
        EXPECT(subset_exact(good, good.size(), sel, 4096, &got, &need) == SICN_EINVAL && need == 0);
        EXPECT(subset_exact(good, good.size(), sel, -1, nullptr, &need) == SICN_EINVAL);
    }
    const uint32_t one = 0;
    EXPECT(sicn_archive::subset(nullptr, good.size(), &one, 1, nullptr, 0, &need) == SICN_EINVAL);
    EXPECT(sicn_archive::subset(good.data(), good.size(), nullptr, 1, nullptr, 0, &need) == SICN_EINVAL);
    EXPECT(sicn_archive::subset(good.data(), good.size(), &one, 1, nullptr, 0, nullptr) == SICN_EINVAL);
    // the index's padding is part of the format: 6 entries are 24 bytes of index and 8 of padding
    Bytes padded = make(pattern({17, 40, 0, 16, 1, 33}), 3, 2, 7);
    EXPECT(subset_exact(padded, padded.size(), {2}, 4096, &got, &need) == SICN_OK);
    padded[32 + 28] = 1;
    EXPECT(subset_exact(padded, padded.size(), {2}, 4096, &got, &need) == SICN_EINVAL);
}

}  // namespace

int main()
{
    const std::vector<uint32_t> one = {5}, eight = {16, 0, 33, 1, 0, 0, 255, 256}, nine = {1, 2, 3, 4, 5, 6, 7, 8, 9},
                                five = {0, 1, 15, 16, 17}, wide = {300, 0, 17, 4, 9, 1000, 16, 15, 0, 0, 0, 0};
    check_selection(one, 1, 1, {0});
    check_selection({0}, 1, 1, {0});
    check_selection(five, 5, 1, {0});
    check_selection(five, 5, 1, {4});
    check_selection(five, 5, 1, {0, 1, 2, 3, 4});
    check_selection(five, 5, 1, {0, 2, 4});
    check_selection(five, 5, 1, {1, 3});
    check_selection(eight, 4, 2, {0});
    check_selection(eight, 4, 2, {2});                          // an image of two empty containers
    check_selection(eight, 4, 2, {1, 3});
    check_selection(eight, 4, 2, {0, 1, 2, 3});
    check_selection(nine, 3, 3, {1});
    check_selection(nine, 3, 3, {0, 2});
    check_selection(wide, 3, 4, {2});                           // only empty containers: a bare header and index
    check_selection(wide, 3, 4, {0, 1});
    std::vector<uint32_t> many(2 * 257);
    for (size_t e = 0; e < many.size(); e++) many[e] = (uint32_t)(e * 37 % 50);
    std::vector<uint32_t> every_other;
    for (uint32_t i = 0; i < 257; i += 2) every_other.push_back(i);
    check_selection(many, 257, 2, every_other);
    check_selection(many, 257, 2, {256});
    check_hostile();
    std::printf("archive_subset_check ok: %d checks\n", checks);
    return 0;
}
