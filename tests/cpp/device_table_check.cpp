// Stand-alone check of csrc/device_table.hpp (the owned device tables, the item -> owner map, the one create path and the workspace
// check of the ragged objects) for builds with the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all device_table_check.cpp -o device_table_check
// The three device calls the header makes are host fakes declared HERE, before the header: they count the live allocations and
// can be told to fail the N-th hipMalloc or the N-th hipMemcpy, which is how the failure paths of a create — out of reach on a
// device that has memory — are walked one by one.  "Device" memory is heap memory of exactly the size asked for, so a copy past
// its end, a double free or a free of a pointer the header never got is an AddressSanitizer report.  Exit status 0 and one line
// "device_table_check ok: <n> checks" when everything held.  No device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };

namespace {
int live = 0, mallocs = 0, copies = 0;       // allocations not yet freed; calls so far
int fail_malloc = 0, fail_copy = 0;          // the call (1-based) that fails, 0 = none
}

hipError_t hipMalloc(void **p, size_t bytes)
{
    if (++mallocs == fail_malloc) {
        *p = reinterpret_cast<void *>(0x10);   // what a failed call leaves behind is not the header's to free
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes);
    live++;
    return hipSuccess;
}

hipError_t hipFree(void *p)
{
    std::free(p);
    live--;
    return hipSuccess;
}

hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind)
{
    if (++copies == fail_copy) return hipErrorUnknown;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}

#include "../../simple_image_compression_network_amd/csrc/device_table.hpp"

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

using sicn::DeviceTable;
using sicn::ItemMap;

void reset(int malloc_n = 0, int copy_n = 0)
{
    mallocs = copies = 0;
    fail_malloc = malloc_n;
    fail_copy = copy_n;
}

// an object as the ragged ones are: three tables, the third the map of a grid
struct Rows { uint64_t off; uint32_t n, first; };
struct Object {
    DeviceTable<Rows> rows;
    DeviceTable<int8_t> bytes;
    DeviceTable<uint32_t> item_owner;
    unsigned items = 0;
};

int build(Object &o)
{
    const std::vector<Rows> rows = {{0, 2, 0}, {64, 0, 2}, {128, 3, 2}};
    const std::vector<int8_t> bytes(37, (int8_t)-5);
    ItemMap map;
    for (size_t i = 0; i < rows.size(); i++) map.add(rows[i].n, (uint32_t)i);
    o.items = (unsigned)map.size();
    return o.rows.upload(rows) && o.bytes.upload(bytes) && map.upload(o.item_owner) ? SICN_OK : SICN_ENOMEM;
}

void create_paths()
{
    // success, then delete
    reset();
    Object *obj = nullptr;
    EXPECT(sicn::make_object(&obj, build) == SICN_OK);
    EXPECT(obj && live == 3 && mallocs == 3 && copies == 3);
    EXPECT(obj->rows.size() == 3 && obj->bytes.size() == 37 && obj->item_owner.size() == 5 && obj->items == 5);
    EXPECT(obj->rows.get()[2].off == 128 && obj->bytes.get()[36] == -5 && obj->item_owner.get()[4] == 2);
    delete obj;
    EXPECT(live == 0);

    // every allocation and every copy fails in its turn
    for (int kind = 0; kind < 2; kind++)
        for (int n = 1; n <= 3; n++) {
            reset(kind == 0 ? n : 0, kind == 1 ? n : 0);
            obj = reinterpret_cast<Object *>(0x20);
            EXPECT(sicn::make_object(&obj, build) == SICN_ENOMEM);
            EXPECT(obj == nullptr);
            EXPECT(live == 0);
            EXPECT(mallocs == n && copies == (kind == 0 ? n - 1 : n));   // nothing is tried behind the failure
        }

    // build's own code comes back, and what it had uploaded goes
    reset();
    obj = reinterpret_cast<Object *>(0x20);
    EXPECT(sicn::make_object(&obj, [](Object &o) { return build(o) ? SICN_ENOMEM : SICN_ENODEV; }) == SICN_ENODEV);
    EXPECT(obj == nullptr && live == 0 && mallocs == 3);

    // a build that runs out of host memory half way
    reset();
    obj = reinterpret_cast<Object *>(0x20);
    EXPECT(sicn::make_object(&obj, [](Object &o) -> int {
               const std::vector<int8_t> bytes(5, (int8_t)1);
               if (!o.bytes.upload(bytes)) return SICN_ENOMEM;
               throw std::bad_alloc();
           }) == SICN_ENOMEM);
    EXPECT(obj == nullptr && live == 0 && mallocs == 1);

    // no place for the result: refused before anything is made
    reset();
    EXPECT(sicn::make_object((Object **)nullptr, build) == SICN_EINVAL);
    EXPECT(mallocs == 0 && live == 0);
}

void tables()
{
    reset();
    {
        DeviceTable<uint32_t> t;
        EXPECT(t.get() == nullptr && t.size() == 0);
        EXPECT(t.upload(std::vector<uint32_t>()));          // an empty vector: success, nothing allocated, the table stays null
        EXPECT(t.get() == nullptr && t.size() == 0 && mallocs == 0 && copies == 0 && live == 0);
        EXPECT(t.upload(nullptr, 0) && mallocs == 0);

        const std::vector<uint32_t> v = {7, 8, 9};
        EXPECT(t.upload(v) && live == 1 && t.size() == 3 && t.get()[1] == 8 && t.mut() == t.get());
        DeviceTable<uint32_t> u(std::move(t));              // a moved-from table is null and frees nothing
        EXPECT(t.get() == nullptr && t.size() == 0 && u.size() == 3 && u.get()[2] == 9 && live == 1);
        DeviceTable<uint32_t> w;
        w = std::move(u);
        EXPECT(u.get() == nullptr && w.get()[0] == 7 && live == 1);
        const std::vector<uint32_t> again = {1};
        EXPECT(w.upload(again) && live == 1 && w.size() == 1 && w.get()[0] == 1);   // the earlier array went
        EXPECT(w.upload(std::vector<uint32_t>()) && live == 0 && w.get() == nullptr);
        EXPECT(w.upload(v) && live == 1);
    }
    EXPECT(live == 0);

    // the copy fails: the memory is the table's and goes with it
    reset(0, 1);
    {
        DeviceTable<uint32_t> t;
        const std::vector<uint32_t> v = {1, 2};
        EXPECT(!t.upload(v) && live == 1);
    }
    EXPECT(live == 0);
    // the allocation fails: the table holds nothing, whatever the call left in the pointer
    reset(1, 0);
    {
        DeviceTable<uint32_t> t;
        const std::vector<uint32_t> v = {1, 2};
        EXPECT(!t.upload(v) && t.get() == nullptr && live == 0);
    }
    EXPECT(live == 0);

    // tables in a vector that grows (sicn_ragged_net::owned)
    reset();
    {
        std::vector<DeviceTable<int8_t>> owned;
        for (int i = 0; i < 9; i++) {
            DeviceTable<int8_t> t;
            const std::vector<int8_t> v((size_t)i + 1, (int8_t)i);
            EXPECT(t.upload(v));
            owned.push_back(std::move(t));
        }
        EXPECT(live == 9 && owned[8].size() == 9 && owned[3].get()[3] == 3);
    }
    EXPECT(live == 0);
}

void item_map()
{
    const size_t counts[] = {0, 1, 3, 0, 2};
    const uint32_t firsts[] = {0, 0, 1, 4, 4};
    ItemMap map;
    std::vector<uint32_t> loop;
    EXPECT(map.size() == 0);
    for (uint32_t i = 0; i < 5; i++) {
        EXPECT(map.add(counts[i], i) == firsts[i]);         // the running first item
        loop.insert(loop.end(), counts[i], i);
    }
    EXPECT(map.size() == 6 && loop.size() == 6);
    reset();
    {
        DeviceTable<uint32_t> t;
        EXPECT(map.upload(t) && t.size() == 6 && live == 1);
        EXPECT(std::memcmp(t.get(), loop.data(), 6 * sizeof(uint32_t)) == 0);   // the map is the insert loop's
        EXPECT(ItemMap().upload(t) && t.get() == nullptr && live == 0);   // an empty grid has no table
    }
    EXPECT(live == 0);
}

void workspace()
{
    alignas(16) static unsigned char block[64];
    EXPECT(sicn::workspace_rc(block, 64, 64) == SICN_OK);
    EXPECT(sicn::workspace_rc(block, 64, 0) == SICN_OK);
    EXPECT(sicn::workspace_rc(nullptr, 64, 0) == SICN_ENOSPC);
    EXPECT(sicn::workspace_rc(block, 63, 64) == SICN_ENOSPC);
    EXPECT(sicn::workspace_rc(block + 8, 56, 16) == SICN_EINVAL);
    EXPECT(sicn::workspace_rc(block + 1, 63, 16) == SICN_EINVAL);
    EXPECT(sicn::workspace_rc(block + 8, 8, 16) == SICN_ENOSPC);   // too small AND misaligned: the size speaks first
}

}  // namespace

int main()
{
    create_paths();
    tables();
    item_map();
    workspace();
    std::printf("device_table_check ok: %lld checks\n", checks);
    return 0;
}
