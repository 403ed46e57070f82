/*
 * sicn_ragged_archive_select.h — random access into a "SICA" archive (sicn_ragged_archive.h): the containers of a SELECTION of its
 * images unpacked into slot buffers with TWO kernel launches, whatever the number of selected images n and of archived images N is,
 * and the archive of a selection alone made on the host (library 0.11, sicn_version() >= 11).  The format does not change: the
 * index gives every container's size, every offset is a prefix sum of a16(size), so the reader needs nothing the archive does not
 * already carry.  An archive resident in device memory thereby serves as an image store: any ascending subset is decoded in a
 * fixed launch count, and the bytes copied depend on the selection alone.
 *
 * Status bits of sicn_ragged_archive_status.error as sicn_ragged_archive_unpack_select_async sets them — those of unpack, with
 * two readings that differ:
 *   bit 3  malformed header (as unpack)
 *   bit 4  the header's n_sections is not the object's, or the header's n_images is SMALLER than the object's (the object is made
 *          for the n selected images; the archive may hold any N >= n), or n_images * n_sections is beyond the format's 2^24
 *   bit 5  the tag differs from expected_tag (as unpack)
 *   bit 6  the size of a SELECTED entry exceeds the capacity of the object's slot it goes to; first_bad is in the OBJECT's
 *          numbering, j * n_sections + section for the j-th selected image.  An unselected entry of any size is no error as long
 *          as the sizes add up
 *   bit 7  the sizes of ALL N * n_sections entries do not add up to total_bytes, or total_bytes > in_bytes, or total_bytes is not a
 *          multiple of 16 (as unpack)
 *   bit 8  NEW: the selection is not one — image_index[j] >= N, or image_index[j] <= image_index[j - 1]
 * The whole source archive is validated as unpack validates it, the index's padding included.
 */
#ifndef SICN_RAGGED_ARCHIVE_SELECT_H
#define SICN_RAGGED_ARCHIVE_SELECT_H

#include "sicn_ragged_archive.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device.  The object (sicn_ragged_archive_create) is made for the n SELECTED images: its slot tables are theirs.  The archive may
 * hold any N >= n images.  image_index_dev: [n] u32 in DEVICE memory, strictly ascending, every value < N; SICN_EINVAL when it is
 * NULL or not 4-byte aligned.  Everything else is sicn_ragged_archive_unpack_async's contract: enqueue only, no allocation, no host
 * synchronisation, capturable into a hipGraph (the index array is read when the kernels run, so a replay may find another
 * selection in it), the same workspace (it holds the n * n_sections offsets and sizes of the selection, not the archive's), the same
 * argument checks.  On success container image_index[j], section s lies at the front of slot j of section s and
 * valid_out[s][j] = {0, size}; bytes of a slot behind its container are never written.  Any error refuses everything: no slot byte
 * is written, every valid_out[s][j] = {error, 0}.  Nothing is read beyond in + in_bytes, nor beyond image_index_dev[0 .. n).
 * status.bytes is the SOURCE archive's total_bytes (0 with bits 3 / 4).  Offsets into the archive are 64-bit. */
int sicn_ragged_archive_unpack_select_async(const sicn_ragged_archive *archive, const uint8_t *in, size_t in_bytes,
                                            uint32_t expected_tag, const uint32_t *image_index_dev, uint8_t *const *slot_buffers,
                                            sicn_codec_status *const *valid_out, sicn_ragged_archive_status *status_dev,
                                            void *workspace, size_t workspace_bytes, void *hip_stream);

/* Pure host, no device: the archive of the selected images alone — same tag, same n_sections, n_images = n_selected, containers
 * copied byte for byte; the result is what the format's arithmetic gives for those containers.  out == NULL: only *out_bytes.
 * SICN_ENOSPC when out_capacity is too small (nothing written, *out_bytes = the size needed).  SICN_EINVAL: whatever
 * sicn_ragged_archive_parse refuses, n_selected < 1, an index >= n_images, not strictly ascending, NULL (archive, image_index or
 * out_bytes).  Reads nothing beyond archive + archive_bytes. */
int sicn_ragged_archive_subset(const uint8_t *archive, size_t archive_bytes, const uint32_t *image_index, uint32_t n_selected,
                               uint8_t *out, size_t out_capacity, uint64_t *out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SICN_RAGGED_ARCHIVE_SELECT_H */
