/*
 * sicn_ragged_archive.h — the containers of a ragged batch as ONE contiguous, self-describing byte string, packed on the device
 * from the coders' slot buffers and status arrays as they lie with TWO kernel launches, and unpacked into the slot buffers and
 * `valid` arrays the ragged decoders take with TWO, whatever the number of images is (library 0.10, sicn_version() >= 10).  It is
 * what a ragged batch (sicn_ragged.h) is stored or sent as: the rANS-W coder of sicn_ragged_codec.h gives one section, the
 * hyperprior configuration two (z from sicn_ragged_codec.h, y from sicn_ragged_ctx.h).  No container format changes; what lies in a
 * section is opaque to this file.
 *
 * Format "SICA" v1 (normative).  Little-endian.  A pure function of the containers' bytes, their sizes and a tag.
 *
 *   offset  field
 *   0       magic "SICA" (bytes 53 49 43 41)
 *   4       u16 version = 1
 *   6       u16 n_sections, 1 .. 4  (1: a rANS-W latent batch; 2: hyperprior, z then y)
 *   8       u32 n_images, >= 1, with n_images * n_sections <= 2^24
 *   12      u32 tag: opaque to the library, stored by pack and compared by unpack
 *   16      u64 total_bytes: the whole archive, this header included; a multiple of 16
 *   24      u32 reserved[2]: zero, checked
 *   32      index: u32 size[n_images][n_sections] — entry e = image * n_sections + section — then zero bytes up to the next
 *           multiple of 16
 *   ...     payload: the containers in index order (image-major: one image's sections are adjacent).  Every container begins at
 *           a multiple of 16 from the start of the archive and is followed by zero bytes up to the next multiple of 16, the last
 *           one included.  A container of size 0 takes no bytes.
 *
 * So with a16(x) = x rounded up to a multiple of 16: the payload begins at P = 32 + a16(4 * n_images * n_sections), entry e lies
 * at P + sum over f < e of a16(size[f]), and total_bytes = P + sum over all e of a16(size[e]).  An archive for which this does not
 * hold is malformed.  (The index's zero padding reads like further entries of size 0: n_images alone says where the index ends.)
 * The cost of the alignment is at most 15 bytes per container (a rANS-W stream alone ends in 260 bytes of
 * flush); in return pack and unpack move 16-byte vectors whenever the base pointers are multiples of 16.
 *
 * Data model.  The archive object is generic over where the slots lie: section s is one buffer, image i's slot at slot_offset[s][i]
 * (a multiple of 16) with a capacity of slot_bytes[s][i] < 4 GiB — the arrays sicn_ragged_codec_layout / sicn_ragged_ctx_layout
 * return, one section per coder.  Offsets are 64-bit.  No alignment is asked of the slot buffers or the archive buffer (16-byte
 * aligned ones take the vector path, decided per section); the workspace and the status must be 8-byte aligned.
 *
 * Kernels.  An index kernel of one workgroup (sizes -> offsets by a prefix sum, header and index, every check) and a copy kernel
 * on a flat grid over work items, an item = one chunk of sicn_ragged_archive_chunk_bytes() of one slot's CAPACITY — the grid is
 * fixed at creation and does not depend on the data; an item beyond its container's size returns at once.
 *
 * Limits (SICN_EINVAL): n_images < 1, n_sections outside 1 .. 4, n_images * n_sections > 2^24, a slot of 4 GiB or more, a slot
 * offset that is not a multiple of 16, >= 2^31 - 1 work items in all, a null pointer.  SICN_ENODEV off gfx950 (creation and the two
 * asynchronous calls).
 */
#ifndef SICN_RAGGED_ARCHIVE_H
#define SICN_RAGGED_ARCHIVE_H

#include "sicn.h"
#include "sicn_codec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SICN_RAGGED_ARCHIVE_MAX_SECTIONS 4
#define SICN_RAGGED_ARCHIVE_HEADER_BYTES 32

typedef struct sicn_ragged_archive sicn_ragged_archive;

/* The header of an archive. */
typedef struct sicn_ragged_archive_info {
    uint32_t version, n_sections, n_images, tag;
    uint64_t total_bytes;
    uint64_t payload_offset; /* where the first container begins: 32 + the index rounded up to 16 */
} sicn_ragged_archive_info;

/* In DEVICE memory.  error: the bits below, 0 = success.  first_bad: the lowest entry (image * n_sections + section) that raised
 * bit 0, 1 or 6; 0xFFFFFFFF when no entry did.  bytes: the archive's size (pack: also with bit 2, the size NEEDED; unpack: the
 * header's total_bytes, 0 when the header could not be read).
 *   pack    bit 0  an image's encoder status carried an error: the entry is stored with size 0, so the error stays with its image
 *           bit 1  a status size exceeds its slot's capacity: the entry is stored with size 0
 *           bit 2  out_capacity is smaller than the archive: nothing is written to `out`
 *   unpack  bit 3  malformed header: shorter than 32 bytes, or magic, version or reserved words wrong, or the index's padding not zero
 *           bit 4  n_images or n_sections is not the object's
 *           bit 5  the tag differs from expected_tag
 *           bit 6  an index size exceeds its slot's capacity
 *           bit 7  the sizes do not add up to total_bytes, or total_bytes > in_bytes, or total_bytes is not a multiple of 16
 *   sicn_ragged_archive_unpack_select_async (sicn_ragged_archive_select.h, library 0.11) unpacks a SELECTION of an archive's images
 *   and sets these bits with two differences, stated there: bit 4 means n_sections is not the object's or n_images is SMALLER than
 *   the object's, and bit 8 is new, a selection that is not strictly ascending or names an image the archive does not hold */
typedef struct sicn_ragged_archive_status {
    uint32_t error;
    uint32_t first_bad;
    uint64_t bytes;
} sicn_ragged_archive_status;

/* ---- pure host, no device ---- */

/* The format's arithmetic.  sizes: [n_images][n_sections].  offsets_out_or_null: [n_images][n_sections], where each container
 * begins.  *total_out_or_null: total_bytes.  SICN_EINVAL beyond the format's limits or for sizes == NULL. */
int sicn_ragged_archive_layout(const uint32_t *sizes, uint32_t n_images, uint32_t n_sections, uint64_t *offsets_out_or_null,
                               uint64_t *total_out_or_null);
/* Reads header and index of an archive in HOST memory (e.g. from a file) with every check unpack makes that needs no slot
 * layout (bits 3 and 7, and n_images / n_sections within the format's limits); reads nothing beyond archive + archive_bytes.
 * sizes_out_or_null / offsets_out_or_null: [n_images][n_sections] of the archive — call once with NULL to learn the counts.
 * SICN_EINVAL for anything malformed. */
int sicn_ragged_archive_parse(const uint8_t *archive, size_t archive_bytes, sicn_ragged_archive_info *info_out,
                              uint32_t *sizes_out_or_null, uint64_t *offsets_out_or_null);
/* Bytes of slot capacity one work item of the copy kernel serves (a tuning constant of the library). */
size_t sicn_ragged_archive_chunk_bytes(void);

/* ---- the archive object ---- */

/* slot_offset[s] / slot_bytes[s]: [n_images] of section s.  Uploads the lookup tables to the current device, once.  Synchronous. */
int sicn_ragged_archive_create(int n_images, int n_sections, const uint64_t *const *slot_offset, const uint64_t *const *slot_bytes,
                               sicn_ragged_archive **out);
void sicn_ragged_archive_free(sicn_ragged_archive *archive);
size_t sicn_ragged_archive_workspace_bytes(const sicn_ragged_archive *archive);
/* The archive's size when every container fills its slot: the capacity of `out` that can never give bit 2. */
size_t sicn_ragged_archive_max_bytes(const sicn_ragged_archive *archive);

/* The contract of the ragged coders: enqueue only, no allocation, no host synchronisation, capturable into a hipGraph, one call in
 * flight per workspace.  SICN_ENOSPC (workspace smaller than sicn_ragged_archive_workspace_bytes) and SICN_EINVAL (a NULL
 * argument, a misaligned workspace or status) enqueue nothing.
 *
 * pack: slot_buffers[s] and enc_status[s] (device sicn_codec_status[n_images], as the section's encoder left it) for each of the
 * object's sections -> out[0 .. status.bytes).  Nothing behind status.bytes is written. */
int sicn_ragged_archive_pack_async(const sicn_ragged_archive *archive, const uint8_t *const *slot_buffers,
                                   const sicn_codec_status *const *enc_status, uint32_t tag, uint8_t *out, size_t out_capacity,
                                   sicn_ragged_archive_status *status_dev, void *workspace, size_t workspace_bytes, void *hip_stream);
/* unpack: in[0 .. in_bytes) -> the containers at the front of their slots and valid_out[s][i] = {0, size}, ready for the ragged
 * decoders' valid_dev argument.  The bytes of a slot behind its container are never written.  On ANY error the whole archive is
 * refused: no byte of any slot buffer is written and every valid_out[s][i] = {error, 0}, so that a decoder run afterwards sees
 * empty slots and reports bit 8 per image.  Nothing is read beyond in + in_bytes. */
int sicn_ragged_archive_unpack_async(const sicn_ragged_archive *archive, const uint8_t *in, size_t in_bytes, uint32_t expected_tag,
                                     uint8_t *const *slot_buffers, sicn_codec_status *const *valid_out,
                                     sicn_ragged_archive_status *status_dev, void *workspace, size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_ARCHIVE_H */
