// The "SICA" archive format (include/sicn_ragged_archive.h) on the host: its arithmetic, the parser of header and index, and the
// archive of a selection of an archive's images (include/sicn_ragged_archive_select.h).  Plain
// C++ without HIP, so that it also compiles into a stand-alone program (tests/cpp/archive_parse_check.cpp and archive_subset_check.cpp
// run it under the host sanitizers).  k_ragged_archive.hip wraps these in the extern "C" entry points; the device parser (k_archive_parse) refuses exactly
// the archives this one refuses (given an object of the archive's own counts, slots that are large enough and the archive's tag).  It
// walks the header in this order too, but where this parser returns at the first finding, the device parser goes on inside one
// stage and may report several bits at once: the tag beside bit 7, and bits 6, 7 and the index's padding (bit 3) together.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/sicn.h"
#include "../../include/sicn_ragged_archive.h"
#include "../../include/sicn_ragged_archive_select.h"

namespace sicn_archive {

constexpr uint32_t VERSION = 1;
constexpr uint32_t HEADER_BYTES = SICN_RAGGED_ARCHIVE_HEADER_BYTES;
constexpr uint32_t MAX_SECTIONS = SICN_RAGGED_ARCHIVE_MAX_SECTIONS;
constexpr uint32_t MAX_ENTRIES = 1u << 24;
constexpr uint32_t CHUNK_BYTES = 16384;          // slot capacity per work item of the copy kernel; a multiple of 16
constexpr uint32_t MAGIC = 0x41434953u;          // "SICA" read as a little-endian u32

constexpr uint64_t a16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

inline bool counts_ok(uint64_t n_images, uint64_t n_sections)
{
    return n_images >= 1 && n_images <= MAX_ENTRIES && n_sections >= 1 && n_sections <= MAX_SECTIONS && n_images * n_sections <= MAX_ENTRIES;
}

constexpr uint64_t payload_offset(uint64_t entries) { return HEADER_BYTES + a16(4 * entries); }

// little-endian loads from bytes of any alignment
inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le32(const uint8_t *p) { return le16(p) | le16(p + 2) << 16; }
inline uint64_t le64(const uint8_t *p) { return (uint64_t)le32(p) | (uint64_t)le32(p + 4) << 32; }

inline int layout(const uint32_t *sizes, uint32_t n_images, uint32_t n_sections, uint64_t *offsets, uint64_t *total)
{
    if (!sizes || !counts_ok(n_images, n_sections)) return SICN_EINVAL;
    const uint64_t entries = (uint64_t)n_images * n_sections;
    uint64_t at = payload_offset(entries);           // <= 32 + 2^26, and 2^24 entries below 2^32 + 16 each: no wrap
    for (uint64_t e = 0; e < entries; e++) {
        if (offsets) offsets[e] = at;
        at += a16(sizes[e]);
    }
    if (total) *total = at;
    return SICN_OK;
}

inline int parse(const uint8_t *b, size_t n, sicn_ragged_archive_info *info, uint32_t *sizes, uint64_t *offsets)
{
    if (!b || !info) return SICN_EINVAL;
    memset(info, 0, sizeof *info);
    // bit 3 of unpack: the fixed header
    if (n < HEADER_BYTES) return SICN_EINVAL;
    if (le32(b) != MAGIC || le16(b + 4) != VERSION || le32(b + 24) != 0 || le32(b + 28) != 0) return SICN_EINVAL;
    const uint32_t n_sections = le16(b + 6), n_images = le32(b + 8);
    // bit 4 of unpack compares with an object; here: the format's own limits
    if (!counts_ok(n_images, n_sections)) return SICN_EINVAL;
    const uint64_t entries = (uint64_t)n_images * n_sections, total = le64(b + 16), payload = payload_offset(entries);
    // bit 7 of unpack: total_bytes against the buffer and against the index
    if ((total & 15) || total > n || payload > total) return SICN_EINVAL;
    const uint8_t *index = b + HEADER_BYTES;         // [HEADER_BYTES, payload) lies inside [0, total) and so inside [0, n)
    uint64_t at = payload;
    for (uint64_t e = 0; e < entries; e++) {
        at += a16(le32(index + 4 * e));              // < 2^24 * (2^32 + 16) + payload: no wrap
        if (at > total) return SICN_EINVAL;
    }
    if (at != total) return SICN_EINVAL;
    for (uint64_t q = HEADER_BYTES + 4 * entries; q < payload; q++)   // the index's padding is part of the format: zero
        if (b[q]) return SICN_EINVAL;
    info->version = VERSION;
    info->n_sections = n_sections;
    info->n_images = n_images;
    info->tag = le32(b + 12);
    info->total_bytes = total;
    info->payload_offset = payload;
    at = payload;
    for (uint64_t e = 0; e < entries; e++) {
        const uint32_t size = le32(index + 4 * e);
        if (sizes) sizes[e] = size;
        if (offsets) offsets[e] = at;
        at += a16(size);
    }
    return SICN_OK;
}

inline void put_le32(uint8_t *p, uint32_t v)
{
    for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}

// The archive of the selected images alone (sicn_ragged_archive_subset).  Two walks over the SOURCE index with a cursor into the
// ascending selection, no allocation: the first gives the size, the second writes.  Everything it reads was vouched for by parse.
inline int subset(const uint8_t *b, size_t n, const uint32_t *image_index, uint32_t n_selected, uint8_t *out, size_t out_capacity,
                  uint64_t *out_bytes)
{
    if (!b || !image_index || !out_bytes) return SICN_EINVAL;
    *out_bytes = 0;
    sicn_ragged_archive_info info;
    if (int rc = parse(b, n, &info, nullptr, nullptr)) return rc;
    if (n_selected < 1 || n_selected > info.n_images) return SICN_EINVAL;
    for (uint32_t j = 0; j < n_selected; j++)
        if (image_index[j] >= info.n_images || (j && image_index[j] <= image_index[j - 1])) return SICN_EINVAL;
    const uint32_t k = info.n_sections;
    const uint64_t entries = (uint64_t)n_selected * k, payload = payload_offset(entries);
    const uint8_t *index = b + HEADER_BYTES;
    uint64_t total = payload;
    for (uint32_t j = 0; j < n_selected; j++)
        for (uint32_t s = 0; s < k; s++) total += a16(le32(index + 4 * ((uint64_t)image_index[j] * k + s)));
    *out_bytes = total;                              // <= the source's total_bytes: fewer index entries, a subset of its containers
    if (!out) return SICN_OK;
    if (out_capacity < total) return SICN_ENOSPC;
    memcpy(out, b, HEADER_BYTES);                    // magic, version, n_sections, tag, reserved
    put_le32(out + 8, n_selected);
    put_le32(out + 16, (uint32_t)total);
    put_le32(out + 20, (uint32_t)(total >> 32));
    memset(out + HEADER_BYTES, 0, (size_t)(payload - HEADER_BYTES));
    uint64_t from = info.payload_offset, to = payload;
    uint32_t j = 0;
    for (uint32_t img = 0; j < n_selected; img++) {  // image_index[n_selected - 1] < n_images ends it
        const bool taken = img == image_index[j];
        for (uint32_t s = 0; s < k; s++) {
            const uint32_t size = le32(index + 4 * ((uint64_t)img * k + s));
            if (taken) {
                put_le32(out + HEADER_BYTES + 4 * ((uint64_t)j * k + s), size);
                if (size) memcpy(out + to, b + from, size);
                memset(out + to + size, 0, (size_t)(a16(size) - size));
                to += a16(size);
            }
            from += a16(size);
        }
        j += taken;
    }
    return SICN_OK;
}

}  // namespace sicn_archive
