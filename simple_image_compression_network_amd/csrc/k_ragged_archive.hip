// Ragged archive (include/sicn_ragged_archive.h): the containers of a ragged batch as one "SICA" byte string, two launches to pack
// it from the coders' slot buffers and status arrays, two to unpack it into slot buffers and `valid` arrays.  The format's host
// arithmetic and host parser are archive_host.hpp.
//
// k_archive_index / k_archive_parse: ONE workgroup.  It walks the n_images * n_sections entries in passes of 256 with a running
//   exclusive prefix of a16(size) (wave scans, the four wave totals through LDS, a carry across passes), TWICE: the first walk only
//   checks and sums — so bit 2 leaves `out` untouched and a refused archive publishes nothing — the second writes the entries'
//   64-bit archive offsets and sizes to the workspace and, packing, the index; unpacking, the `valid` arrays.
// k_archive_copy<PACK>: flat grid over work items, an item = CHUNK bytes of one entry's slot CAPACITY, so the grid is fixed at
//   creation.  Two tables, built on the host at creation, as in the ragged crop (k_ragged.hip):
//     item_entry[item] : the entry an item belongs to
//     rows[entry]      : { slot_off, slot_bytes, first_item, section }
//   Both loads depend on blockIdx.x only and stay in scalar registers.  An item whose chunk begins at or beyond the entry's actual
//   size returns at once.  `vecmask` bit s (per launch, host-made): section s's slot buffer and the archive buffer are both 16-byte
//   aligned; then — slot offsets and archive offsets being multiples of 16 by construction — a chunk moves as uint4, 4 per lane,
//   and only the container's last partial 16 bytes move bytewise.  Otherwise byte by byte.
// k_archive_parse_select (include/sicn_ragged_archive_select.h): k_archive_parse for an object made for a SELECTION of the archive's
//   images; then k_archive_copy<false> as it is, over the object's item grid.  Described at the kernel.
#include <vector>

#include "archive_host.hpp"
#include "device_table.hpp"
#include "k_ragged_common.hpp"
#include "sicn_internal.h"

namespace {

using namespace sicn_archive;

constexpr uint32_t REFUSED = 0xFCu;          // pack: bit 2; unpack: bits 3 .. 7 — the copy kernel moves nothing
constexpr uint32_t NO_ENTRY = 0xFFFFFFFFu;
constexpr int WG = 256;

struct ArchRow {
    uint64_t slot_off;
    uint32_t slot_bytes, first_item, section, pad;
};
struct Ptrs4 { uint8_t *p[MAX_SECTIONS]; };        // one pointer per section, by value in the kernel arguments

// a select chain, not an indexed load: kernel arguments indexed at run time would go through scratch
__device__ __forceinline__ uint8_t *pick(const Ptrs4 &a, uint32_t s) { return s == 0 ? a.p[0] : s == 1 ? a.p[1] : s == 2 ? a.p[2] : a.p[3]; }

// little-endian words at any alignment; al4: the base pointer is a multiple of 4 (wave-uniform)
__device__ __forceinline__ uint32_t load32(const uint8_t *p, bool al4)
{
    if (al4) return *reinterpret_cast<const uint32_t *>(p);
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
__device__ __forceinline__ void store32(uint8_t *p, uint32_t v, bool al4)
{
    if (al4) { *reinterpret_cast<uint32_t *>(p) = v; return; }
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// One walk over the entries by the whole workgroup: put(e, size, offset) with offset = start + sum over f < e of a16(get(f)).
// Returns start + the sum over all entries, in every thread.  Ends with a barrier.  wave_total: WG / 64 words of LDS, the kernel's
// (declared here, every instantiation of the template would get its own).
template <class Get, class Put>
__device__ __forceinline__ uint64_t walk(uint64_t *wave_total, uint32_t entries, uint64_t start, Get get, Put put)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = start;
    for (uint32_t base = 0; base < entries; base += WG) {         // entries <= 2^24: base + WG cannot wrap
        const uint32_t e = base + threadIdx.x;
        const bool live = e < entries;
        const uint32_t size = live ? get(e) : 0;
        const uint64_t mine = a16(size);
        uint64_t incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t up = __shfl_up((unsigned long long)incl, d, 64);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        uint64_t before = 0, all = 0;
        for (uint32_t w = 0; w < WG / 64; w++) {
            const uint64_t t = wave_total[w];
            if (w < wave) before += t;
            all += t;
        }
        if (live) put(e, size, carry + before + incl - mine);
        carry += all;
        __syncthreads();
    }
    return carry;
}

// error bits and the lowest guilty entry of all threads -> every thread.  Ends with a barrier.
__device__ __forceinline__ void gather(uint32_t &err, uint32_t &bad)
{
    __shared__ uint32_t s_err, s_bad;
    if (threadIdx.x == 0) { s_err = 0; s_bad = NO_ENTRY; }
    __syncthreads();
    if (err) atomicOr(&s_err, err);
    if (bad != NO_ENTRY) atomicMin(&s_bad, bad);
    __syncthreads();
    err = s_err;
    bad = s_bad;
    __syncthreads();
}

__global__ __launch_bounds__(WG) void k_archive_index(Ptrs4 enc_status, const ArchRow *__restrict__ rows, uint32_t n_images, uint32_t k,
                                                      uint32_t tag, uint8_t *__restrict__ out, uint64_t out_capacity,
                                                      sicn_ragged_archive_status *__restrict__ status, uint64_t *__restrict__ ws_off,
                                                      uint32_t *__restrict__ ws_size)
{
    __shared__ uint64_t wave_total[WG / 64];
    const uint32_t entries = n_images * k;
    const uint64_t payload = payload_offset(entries);
    uint32_t err = 0, bad = NO_ENTRY;
    // walk 1: the sizes as they will be stored, into the workspace, and their sum
    const uint64_t total = walk(wave_total, entries, payload,
        [&](uint32_t e) {
            const uint32_t img = e / k, s = e - img * k;
            const uint32_t *st = reinterpret_cast<const uint32_t *>(pick(enc_status, s)) + 2 * (size_t)img;   // sicn_codec_status {error, bytes}
            uint32_t size = st[1], mine = 0;
            if (st[0]) mine |= 1u;
            if (size > rows[e].slot_bytes) mine |= 2u;
            if (mine) { err |= mine; bad = min(bad, e); size = 0; }
            ws_size[e] = size;
            return size;
        },
        [](uint32_t, uint32_t, uint64_t) {});
    gather(err, bad);
    if (total > out_capacity) err |= 4u;
    if (threadIdx.x == 0) {
        status->error = err;
        status->first_bad = bad;
        status->bytes = total;
    }
    if (err & 4u) return;                                    // nothing was written to `out`
    const bool al4 = (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    if (threadIdx.x < HEADER_BYTES / 4) {
        const uint32_t words[HEADER_BYTES / 4] = {MAGIC, VERSION | k << 16, n_images, tag, (uint32_t)total, (uint32_t)(total >> 32), 0u, 0u};
        uint32_t v = 0;
        for (uint32_t i = 0; i < HEADER_BYTES / 4; i++) v = threadIdx.x == i ? words[i] : v;
        store32(out + 4 * threadIdx.x, v, al4);
    }
    if (threadIdx.x < (payload - HEADER_BYTES) / 4 - entries)  // the index's padding: 0 .. 3 words
        store32(out + HEADER_BYTES + 4 * ((size_t)entries + threadIdx.x), 0u, al4);
    // walk 2: offsets into the workspace, the index into the archive.  Thread t reads the ws_size entries it wrote itself.
    walk(wave_total, entries, payload, [&](uint32_t e) { return ws_size[e]; },
         [&](uint32_t e, uint32_t size, uint64_t off) {
             ws_off[e] = off;
             store32(out + HEADER_BYTES + 4 * (size_t)e, size, al4);
         });
}

__global__ __launch_bounds__(WG) void k_archive_parse(const uint8_t *__restrict__ in, uint64_t in_bytes, uint32_t expected_tag,
                                                      const ArchRow *__restrict__ rows, uint32_t n_images, uint32_t k, Ptrs4 valid,
                                                      sicn_ragged_archive_status *__restrict__ status, uint64_t *__restrict__ ws_off,
                                                      uint32_t *__restrict__ ws_size)
{
    __shared__ uint64_t wave_total[WG / 64];
    const uint32_t entries = n_images * k;
    const uint64_t payload = payload_offset(entries);
    const bool al4 = (reinterpret_cast<uintptr_t>(in) & 3) == 0;
    const uint8_t *index = in + HEADER_BYTES;
    uint32_t err = 0, bad = NO_ENTRY;
    uint64_t total = 0;
    // the checks of sicn_archive::parse, stage by stage in its order (the bits of one stage may come together); every thread reads the header itself (uniform)
    if (in_bytes < HEADER_BYTES) err |= 8u;
    else if (load32(in, al4) != MAGIC || (load32(in + 4, al4) & 0xFFFFu) != VERSION || load32(in + 24, al4) != 0 || load32(in + 28, al4) != 0) err |= 8u;
    if (!err) {
        if ((load32(in + 4, al4) >> 16) != k || load32(in + 8, al4) != n_images) err |= 16u;
    }
    if (!err) {                                              // the header is sound and the index has the object's shape
        total = (uint64_t)load32(in + 16, al4) | (uint64_t)load32(in + 20, al4) << 32;
        if (load32(in + 12, al4) != expected_tag) err |= 32u;
        if ((total & 15) || total > in_bytes || payload > total) err |= 128u;
        if (!(err & 128u)) {                                 // [32, payload) lies inside [0, total) and so inside [0, in_bytes)
            const uint64_t sum = walk(wave_total, entries, payload,
                [&](uint32_t e) {
                    const uint32_t size = load32(index + 4 * (size_t)e, al4);
                    if (size > rows[e].slot_bytes) { err |= 64u; bad = min(bad, e); }
                    return size;
                },
                [](uint32_t, uint32_t, uint64_t) {});
            if (threadIdx.x < (payload - HEADER_BYTES) / 4 - entries && load32(index + 4 * ((size_t)entries + threadIdx.x), al4) != 0) err |= 8u;
            gather(err, bad);
            if (sum != total) err |= 128u;
        }
    }
    if (threadIdx.x == 0) {
        status->error = err;
        status->first_bad = bad;
        status->bytes = (err & 24u) ? 0 : total;
    }
    if (err) {                                               // refused: every slot is empty for the decoders
        for (uint32_t e = threadIdx.x; e < entries; e += WG) {
            const uint32_t img = e / k, s = e - img * k;
            uint32_t *v = reinterpret_cast<uint32_t *>(pick(valid, s)) + 2 * (size_t)img;
            v[0] = err;
            v[1] = 0;
        }
        return;
    }
    walk(wave_total, entries, payload, [&](uint32_t e) { return load32(index + 4 * (size_t)e, al4); },
         [&](uint32_t e, uint32_t size, uint64_t off) {
             const uint32_t img = e / k, s = e - img * k;
             uint32_t *v = reinterpret_cast<uint32_t *>(pick(valid, s)) + 2 * (size_t)img;
             v[0] = 0;
             v[1] = size;
             ws_off[e] = off;
             ws_size[e] = size;
         });
}

// The parser of sicn_ragged_archive_unpack_select_async (include/sicn_ragged_archive_select.h): k_archive_parse for an object made for
// the n_sel SELECTED images of an archive of N >= n_sel.  The prefix sum runs over all N * k entries of the source index, pass by
// pass through `walk`; what is written — ws_off / ws_size / valid, in the OBJECT's numbering j * k + section — is written for the
// selected entries alone.  "Is this source image selected, and as which j" costs one coalesced load per thread and pass: the
// selection ascends, so the selected images of a pass are the next ones behind a workgroup-uniform cursor `cur`, at most WG of
// them (a pass covers at most WG consecutive images).  Thread t loads image_index[cur + t] and, when that image lies in the pass,
// writes cur + t into the pass's LDS window win[image - first image of the pass]; an entry then looks its image up in the window.
// The cursor moves on by the selected images that END in this pass (k = 3: an image may straddle two passes and stays for the next).
template <bool WRITE, class Each>
__device__ __forceinline__ uint64_t walk_selected(uint64_t *wave_total, uint32_t *win, uint32_t *taken, const uint8_t *index, bool al4,
                                                  uint32_t entries, uint32_t k, uint64_t payload, const uint32_t *__restrict__ image_index,
                                                  uint32_t n_sel, Each each)
{
    uint64_t carry = payload;
    uint32_t cur = 0;
    for (uint32_t base = 0; base < entries; base += WG) {
        const uint32_t img0 = base / k, img_next = (base + WG) / k;      // the first image of this pass and of the next
        win[threadIdx.x] = NO_ENTRY;
        if (threadIdx.x == 0) *taken = 0;
        __syncthreads();
        const uint32_t j = cur + threadIdx.x;
        const uint32_t image = j < n_sel ? image_index[j] : NO_ENTRY;    // >= img0: every image below it is behind the cursor
        if (image - img0 < (uint32_t)WG) win[image - img0] = j;
        const uint64_t ends_here = __ballot(image < img_next);
        if ((threadIdx.x & 63) == 0 && ends_here) atomicAdd(taken, (uint32_t)__popcll(ends_here));
        __syncthreads();
        cur = uni(cur + *taken);
        const uint32_t count = entries - base < (uint32_t)WG ? entries - base : (uint32_t)WG;
        uint32_t oe = NO_ENTRY, sel = NO_ENTRY, section = 0;              // this thread's entry in the object's numbering: oe = sel * k + section
        carry = walk(wave_total, count, carry,
            [&](uint32_t t) {
                const uint32_t e = base + t, img = e / k;
                const uint32_t size = load32(index + 4 * (size_t)e, al4);
                section = e - img * k;
                sel = win[img - img0];
                oe = sel == NO_ENTRY ? NO_ENTRY : sel * k + section;
                if (!WRITE && oe != NO_ENTRY) each(oe, sel, section, size, (uint64_t)0);
                return size;
            },
            [&](uint32_t, uint32_t size, uint64_t off) {
                if (WRITE && oe != NO_ENTRY) each(oe, sel, section, size, off);
            });
    }
    return carry;
}

__global__ __launch_bounds__(WG) void k_archive_parse_select(const uint8_t *__restrict__ in, uint64_t in_bytes, uint32_t expected_tag,
                                                             const ArchRow *__restrict__ rows, uint32_t n_sel, uint32_t k,
                                                             const uint32_t *__restrict__ image_index, Ptrs4 valid,
                                                             sicn_ragged_archive_status *__restrict__ status,
                                                             uint64_t *__restrict__ ws_off, uint32_t *__restrict__ ws_size)
{
    __shared__ uint64_t wave_total[WG / 64];
    __shared__ uint32_t win[WG], taken;
    const bool al4 = (reinterpret_cast<uintptr_t>(in) & 3) == 0;
    const uint8_t *index = in + HEADER_BYTES;
    uint32_t err = 0, bad = NO_ENTRY, n_images = 0;
    uint64_t total = 0;
    // k_archive_parse's stages in its order; the object's counts are the selection's, the archive's come from its header
    if (in_bytes < HEADER_BYTES) err |= 8u;
    else if (load32(in, al4) != MAGIC || (load32(in + 4, al4) & 0xFFFFu) != VERSION || load32(in + 24, al4) != 0 || load32(in + 28, al4) != 0) err |= 8u;
    if (!err) {
        n_images = load32(in + 8, al4);
        if ((load32(in + 4, al4) >> 16) != k || n_images < n_sel || n_images > MAX_ENTRIES / k) err |= 16u;
    }
    if (!err) {                                              // the header is sound and the index can hold the selection
        const uint32_t entries = n_images * k;               // <= 2^24
        const uint64_t payload = payload_offset(entries);
        total = (uint64_t)load32(in + 16, al4) | (uint64_t)load32(in + 20, al4) << 32;
        if (load32(in + 12, al4) != expected_tag) err |= 32u;
        if ((total & 15) || total > in_bytes || payload > total) err |= 128u;
        for (uint32_t j = threadIdx.x; j < n_sel; j += WG) {  // the selection: image_index[0 .. n_sel) and nothing else
            const uint32_t image = image_index[j];
            if (image >= n_images || (j && image <= image_index[j - 1])) err |= 256u;
        }
        gather(err, bad);                                    // from here on err is the same in every thread
        if (!(err & (128u | 256u))) {                        // [32, payload) lies inside [0, in_bytes), and the window can trust the selection
            const uint64_t sum = walk_selected<false>(wave_total, win, &taken, index, al4, entries, k, payload, image_index, n_sel,
                [&](uint32_t oe, uint32_t, uint32_t, uint32_t size, uint64_t) {
                    if (size > rows[oe].slot_bytes) { err |= 64u; bad = min(bad, oe); }
                });
            if (threadIdx.x < (payload - HEADER_BYTES) / 4 - entries && load32(index + 4 * ((size_t)entries + threadIdx.x), al4) != 0) err |= 8u;
            gather(err, bad);
            if (sum != total) err |= 128u;
        }
    }
    if (threadIdx.x == 0) {
        status->error = err;
        status->first_bad = bad;
        status->bytes = (err & 24u) ? 0 : total;
    }
    if (err) {                                               // refused: every slot is empty for the decoders, and for the copy kernel —
        for (uint32_t e = threadIdx.x; e < n_sel * k; e += WG) {   // bit 8 is not in its REFUSED mask, an entry of size 0 has no item to move
            const uint32_t img = e / k, s = e - img * k;
            uint32_t *v = reinterpret_cast<uint32_t *>(pick(valid, s)) + 2 * (size_t)img;
            v[0] = err;
            v[1] = 0;
            ws_size[e] = 0;
        }
        return;
    }
    walk_selected<true>(wave_total, win, &taken, index, al4, n_images * k, k, payload_offset(n_images * k), image_index, n_sel,
        [&](uint32_t oe, uint32_t sel, uint32_t section, uint32_t size, uint64_t off) {
            uint32_t *v = reinterpret_cast<uint32_t *>(pick(valid, section)) + 2 * (size_t)sel;
            v[0] = 0;
            v[1] = size;
            ws_off[oe] = off;
            ws_size[oe] = size;
        });
}

template <bool PACK>
__global__ __launch_bounds__(WG) void k_archive_copy(Ptrs4 slots, uint8_t *__restrict__ arch, const ArchRow *__restrict__ rows,
                                                     const uint32_t *__restrict__ item_entry, uint32_t n_items,
                                                     const uint64_t *__restrict__ ws_off, const uint32_t *__restrict__ ws_size,
                                                     const sicn_ragged_archive_status *__restrict__ status, uint32_t vecmask)
{
    const uint32_t item = blockIdx.x;
    if (item >= n_items) return;                             // an object without any slot capacity still launches one workgroup
    if (uni(status->error) & REFUSED) return;
    const uint32_t e = uni(item_entry[item]);
    const ArchRow *row = rows + e;
    const uint32_t size = uni(ws_size[e]);
    const uint32_t chunk0 = (item - uni(row->first_item)) * CHUNK_BYTES;   // < slot_bytes < 2^32
    if (chunk0 >= size) return;
    const uint32_t len = size - chunk0 < CHUNK_BYTES ? size - chunk0 : CHUNK_BYTES;
    const uint32_t section = uni(row->section);
    // 64-bit between entries, 32-bit inside the item
    uint8_t *s = pick(slots, section) + uni(row->slot_off) + chunk0;
    uint8_t *a = arch + uni(ws_off[e]) + chunk0;
    if ((vecmask >> section) & 1u) {
        constexpr uint32_t PER = CHUNK_BYTES / 16 / WG;      // 4 vectors per lane
        static_assert(PER * 16 * WG == CHUNK_BYTES, "a chunk is a whole number of 16-byte vectors per lane");
        const uint32_t nvec = len / 16, tail = len & 15;     // tail: only behind a container's end
        // a slot buffer and the archive buffer never overlap: said here, because a section pointer picked at run time tells the
        // compiler nothing, and it would otherwise wait for each load before the store behind it
        const uint4 *__restrict__ from = reinterpret_cast<const uint4 *>(PACK ? s : a);
        uint4 *__restrict__ to = reinterpret_cast<uint4 *>(PACK ? a : s);
        if (nvec == PER * WG) {                              // a whole chunk: every load in flight before the first store
            static_assert(PER == 4, "four named vectors: an array here was promoted to LDS");
            const uint32_t i = threadIdx.x;
            const uint4 v0 = from[i], v1 = from[i + WG], v2 = from[i + 2 * WG], v3 = from[i + 3 * WG];
            asm volatile("" ::: "memory");                   // left to itself the scheduler pairs each load with its store and waits four times
            to[i] = v0;
            to[i + WG] = v1;
            to[i + 2 * WG] = v2;
            to[i + 3 * WG] = v3;
        } else {
            for (uint32_t i = threadIdx.x; i < nvec; i += WG) to[i] = from[i];
        }
        if (tail && threadIdx.x < 16) {
            const uint32_t at = nvec * 16 + threadIdx.x;
            if (PACK) a[at] = threadIdx.x < tail ? s[at] : (uint8_t)0;   // ... and the zero padding up to the next multiple of 16
            else if (threadIdx.x < tail) s[at] = a[at];
        }
    } else {
        for (uint32_t i = threadIdx.x; i < len; i += WG) {
            if (PACK) a[i] = s[i];
            else s[i] = a[i];
        }
        if (PACK && chunk0 + len == size && threadIdx.x < ((16u - (size & 15u)) & 15u)) a[len + threadIdx.x] = 0;
    }
}

}  // namespace

struct sicn_ragged_archive {
    uint32_t n_images = 0, k = 0, entries = 0, items = 0;
    uint64_t max_bytes = 0, ws_bytes = 0;
    sicn::DeviceTable<ArchRow> d_rows;              // [entries]
    sicn::DeviceTable<uint32_t> d_item_entry;       // [max(items, 1)]
};

extern "C" int sicn_ragged_archive_layout(const uint32_t *sizes, uint32_t n_images, uint32_t n_sections, uint64_t *offsets_out_or_null,
                                          uint64_t *total_out_or_null)
{
    return layout(sizes, n_images, n_sections, offsets_out_or_null, total_out_or_null);
}

extern "C" int sicn_ragged_archive_parse(const uint8_t *archive, size_t archive_bytes, sicn_ragged_archive_info *info_out,
                                         uint32_t *sizes_out_or_null, uint64_t *offsets_out_or_null)
{
    return parse(archive, archive_bytes, info_out, sizes_out_or_null, offsets_out_or_null);
}

extern "C" size_t sicn_ragged_archive_chunk_bytes(void) { return CHUNK_BYTES; }

extern "C" void sicn_ragged_archive_free(sicn_ragged_archive *archive) { delete archive; }

extern "C" int sicn_ragged_archive_create(int n_images, int n_sections, const uint64_t *const *slot_offset, const uint64_t *const *slot_bytes,
                                          sicn_ragged_archive **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    if (n_images < 1 || n_sections < 1 || !counts_ok((uint64_t)n_images, (uint64_t)n_sections) || !slot_offset || !slot_bytes) return SICN_EINVAL;
    for (int s = 0; s < n_sections; s++)
        if (!slot_offset[s] || !slot_bytes[s]) return SICN_EINVAL;
    return sicn::make_object(out, [&](sicn_ragged_archive &ar) {
        ar.n_images = (uint32_t)n_images;
        ar.k = (uint32_t)n_sections;
        ar.entries = ar.n_images * ar.k;
        std::vector<ArchRow> rows((size_t)ar.entries);
        uint64_t items = 0, most = payload_offset(ar.entries);
        for (uint32_t i = 0; i < ar.n_images; i++)
            for (uint32_t s = 0; s < ar.k; s++) {
                const uint64_t off = slot_offset[s][i], cap = slot_bytes[s][i];
                if ((off & 15) || cap > 0xFFFFFFFFull || off + cap < off) return SICN_EINVAL;
                rows[(size_t)i * ar.k + s] = ArchRow{off, (uint32_t)cap, (uint32_t)items, s, 0};
                items += (cap + CHUNK_BYTES - 1) / CHUNK_BYTES;     // <= 2^24 * 2^18
                most += a16(cap);
                if (items >= 0x7fffffffull) return SICN_EINVAL;    // grid.x
            }
        if (int rc = sicn::chip_geom(nullptr)) return rc;       // no device, or not a gfx950 one
        ar.items = (uint32_t)items;
        ar.max_bytes = most;
        ar.ws_bytes = a16(12ull * ar.entries);
        sicn::ItemMap item_entry;
        for (uint32_t e = 0; e < ar.entries; e++) item_entry.add(((size_t)rows[e].slot_bytes + CHUNK_BYTES - 1) / CHUNK_BYTES, e);
        if (!item_entry.size()) item_entry.add(1, 0);
        return ar.d_rows.upload(rows) && item_entry.upload(ar.d_item_entry) ? SICN_OK : SICN_ENOMEM;
    });
}

extern "C" size_t sicn_ragged_archive_workspace_bytes(const sicn_ragged_archive *archive) { return archive ? (size_t)archive->ws_bytes : 0; }
extern "C" size_t sicn_ragged_archive_max_bytes(const sicn_ragged_archive *archive) { return archive ? (size_t)archive->max_bytes : 0; }

namespace {

// the arguments both calls share; ptrs: k section pointers -> Ptrs4, and bit s of *vecmask when it and `arch` are 16-byte aligned
int common_checks(const sicn_ragged_archive *ar, const void *const *a, const void *const *b, const void *arch, const void *status_dev,
                  const void *workspace, size_t workspace_bytes, Ptrs4 *pa, Ptrs4 *pb, uint32_t *vecmask)
{
    if (!ar || !a || !b || !arch || !status_dev) return SICN_EINVAL;
    *pa = Ptrs4{};
    *pb = Ptrs4{};
    *vecmask = 0;
    for (uint32_t s = 0; s < ar->k; s++) {
        if (!a[s] || !b[s]) return SICN_EINVAL;
        pa->p[s] = (uint8_t *)const_cast<void *>(a[s]);
        pb->p[s] = (uint8_t *)const_cast<void *>(b[s]);
        if (((reinterpret_cast<uintptr_t>(a[s]) | reinterpret_cast<uintptr_t>(arch)) & 15) == 0) *vecmask |= 1u << s;
        if (reinterpret_cast<uintptr_t>(b[s]) & 3) return SICN_EINVAL;             // sicn_codec_status arrays
    }
    if (!workspace || workspace_bytes < ar->ws_bytes) return SICN_ENOSPC;
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(status_dev)) & 7) return SICN_EINVAL;
    return sicn::chip_geom(nullptr);
}

}  // namespace

extern "C" int sicn_ragged_archive_pack_async(const sicn_ragged_archive *archive, const uint8_t *const *slot_buffers,
                                              const sicn_codec_status *const *enc_status, uint32_t tag, uint8_t *out, size_t out_capacity,
                                              sicn_ragged_archive_status *status_dev, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    Ptrs4 slots, st;
    uint32_t vecmask;
    if (int rc = common_checks(archive, (const void *const *)slot_buffers, (const void *const *)enc_status, out, status_dev, workspace,
                               workspace_bytes, &slots, &st, &vecmask))
        return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint64_t *ws_off = (uint64_t *)workspace;
    uint32_t *ws_size = (uint32_t *)(ws_off + archive->entries);
    hipLaunchKernelGGL(k_archive_index, dim3(1), dim3(WG), 0, stream, st, archive->d_rows.get(), archive->n_images, archive->k, tag, out,
                       (uint64_t)out_capacity, status_dev, ws_off, ws_size);
    hipLaunchKernelGGL(k_archive_copy<true>, dim3(archive->items ? archive->items : 1u), dim3(WG), 0, stream, slots, out, archive->d_rows.get(),
                       archive->d_item_entry.get(), archive->items, ws_off, ws_size, status_dev, vecmask);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_ragged_archive_unpack_async(const sicn_ragged_archive *archive, const uint8_t *in, size_t in_bytes, uint32_t expected_tag,
                                                uint8_t *const *slot_buffers, sicn_codec_status *const *valid_out,
                                                sicn_ragged_archive_status *status_dev, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    Ptrs4 slots, valid;
    uint32_t vecmask;
    if (int rc = common_checks(archive, (const void *const *)slot_buffers, (const void *const *)valid_out, in, status_dev, workspace,
                               workspace_bytes, &slots, &valid, &vecmask))
        return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint64_t *ws_off = (uint64_t *)workspace;
    uint32_t *ws_size = (uint32_t *)(ws_off + archive->entries);
    hipLaunchKernelGGL(k_archive_parse, dim3(1), dim3(WG), 0, stream, in, (uint64_t)in_bytes, expected_tag, archive->d_rows.get(), archive->n_images,
                       archive->k, valid, status_dev, ws_off, ws_size);
    hipLaunchKernelGGL(k_archive_copy<false>, dim3(archive->items ? archive->items : 1u), dim3(WG), 0, stream, slots, const_cast<uint8_t *>(in),
                       archive->d_rows.get(), archive->d_item_entry.get(), archive->items, ws_off, ws_size, status_dev, vecmask);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_ragged_archive_unpack_select_async(const sicn_ragged_archive *archive, const uint8_t *in, size_t in_bytes,
                                                       uint32_t expected_tag, const uint32_t *image_index_dev, uint8_t *const *slot_buffers,
                                                       sicn_codec_status *const *valid_out, sicn_ragged_archive_status *status_dev,
                                                       void *workspace, size_t workspace_bytes, void *hip_stream)
{
    Ptrs4 slots, valid;
    uint32_t vecmask;
    if (!image_index_dev || (reinterpret_cast<uintptr_t>(image_index_dev) & 3)) return SICN_EINVAL;
    if (int rc = common_checks(archive, (const void *const *)slot_buffers, (const void *const *)valid_out, in, status_dev, workspace,
                               workspace_bytes, &slots, &valid, &vecmask))
        return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint64_t *ws_off = (uint64_t *)workspace;
    uint32_t *ws_size = (uint32_t *)(ws_off + archive->entries);
    hipLaunchKernelGGL(k_archive_parse_select, dim3(1), dim3(WG), 0, stream, in, (uint64_t)in_bytes, expected_tag, archive->d_rows.get(),
                       archive->n_images, archive->k, image_index_dev, valid, status_dev, ws_off, ws_size);
    hipLaunchKernelGGL(k_archive_copy<false>, dim3(archive->items ? archive->items : 1u), dim3(WG), 0, stream, slots, const_cast<uint8_t *>(in),
                       archive->d_rows.get(), archive->d_item_entry.get(), archive->items, ws_off, ws_size, status_dev, vecmask);
    return hipGetLastError() == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_ragged_archive_subset(const uint8_t *archive, size_t archive_bytes, const uint32_t *image_index, uint32_t n_selected,
                                          uint8_t *out, size_t out_capacity, uint64_t *out_bytes)
{
    return subset(archive, archive_bytes, image_index, n_selected, out, out_capacity, out_bytes);
}
