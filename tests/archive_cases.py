"""The "SICA" v1 archive format restated in numpy, from the comment block of include/sicn_ragged_archive.h alone (not from the C
code), and the hostile archives both parsers must refuse.  Shared by tests/test_ragged_archive.py (host) and
tests/test_ragged_archive_gpu.py (device); nothing here touches the library.

    0   "SICA"      4  u16 version = 1      6  u16 n_sections (1 .. 4)      8  u32 n_images      12  u32 tag
    16  u64 total_bytes (a multiple of 16)  24 u32 reserved[2] = 0
    32  u32 size[n_images][n_sections], zero bytes to the next multiple of 16
    ... the containers in index order, each at a multiple of 16 and zero-padded to the next one; size 0 takes no bytes
"""
import struct

import numpy as np

HEADER_BYTES = 32
MAX_SECTIONS = 4
MAX_ENTRIES = 1 << 24
# status bits of include/sicn_ragged_archive.h
PACK_STATUS_ERROR, PACK_OVER_CAPACITY, PACK_NO_ROOM = 1, 2, 4
BAD_HEADER, BAD_COUNTS, BAD_TAG, BAD_SIZE, BAD_TOTAL = 8, 16, 32, 64, 128
NO_ENTRY = 0xFFFFFFFF


def a16(x: int) -> int:
    return -(-int(x) // 16) * 16


def layout(sizes):
    """sizes: [n_images][n_sections] -> (offsets [n_images][n_sections] as a flat list of Python ints, total_bytes)."""
    sizes = np.asarray(sizes, dtype=np.uint64)
    n, k = sizes.shape
    at = HEADER_BYTES + a16(4 * n * k)
    offsets = []
    for s in sizes.reshape(-1).tolist():
        offsets.append(at)
        at += a16(s)
    return offsets, at


def make_archive(containers, tag: int = 0) -> bytes:
    """containers: per image, a sequence of n_sections `bytes` -> the archive."""
    n, k = len(containers), len(containers[0])
    assert all(len(c) == k for c in containers)
    sizes = [[len(b) for b in c] for c in containers]
    offsets, total = layout(sizes)
    out = np.zeros(total, dtype=np.uint8)
    out[:HEADER_BYTES] = np.frombuffer(b"SICA" + struct.pack("<HHIIQII", 1, k, n, tag & 0xFFFFFFFF, total, 0, 0), dtype=np.uint8)
    out[HEADER_BYTES:HEADER_BYTES + 4 * n * k] = np.asarray(sizes, dtype="<u4").reshape(-1).view(np.uint8)
    for off, b in zip(offsets, (b for c in containers for b in c)):
        out[off:off + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return out.tobytes()


def patched(archive: bytes, offset: int, fmt: str, value) -> bytes:
    b = bytearray(archive)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def sample_containers(n: int, k: int, seed: int = 0, sizes=None):
    """Random bytes of the given sizes ([n][k]; default: a spread around the 16-byte steps)."""
    rng = np.random.default_rng(seed)
    spread = [0, 1, 15, 16, 17, 31, 33, 48, 100, 5]
    return [tuple(rng.integers(0, 256, sizes[i][s] if sizes is not None else spread[(i * k + s) % len(spread)], dtype=np.uint8).tobytes()
                  for s in range(k)) for i in range(n)]


def hostile(archive: bytes, n: int, k: int):
    """[(name, bytes, the unpack status bit a device parser of an (n, k) object must raise)] — each from ONE patched field of a
    valid archive of n images and k sections whose entry 1 is not empty and whose index needs no padding.  The host parser answers SICN_EINVAL to every one except
    the tag (it has nothing to compare a tag with)."""
    total = struct.unpack_from("<Q", archive, 16)[0]
    size1 = struct.unpack_from("<I", archive, HEADER_BYTES + 4)[0]
    # an index without padding: behind a padded one, n_images + 1 would read the padding as one more image of empty containers,
    # which IS an archive of the format
    assert total == len(archive) and size1 > 0 and n * k >= 2 and (4 * n * k) % 16 == 0
    cases = [
        ("magic", patched(archive, 0, "<I", 0x42434953), BAD_HEADER),
        ("magic_case", patched(archive, 3, "<B", ord("a")), BAD_HEADER),
        ("version_0", patched(archive, 4, "<H", 0), BAD_HEADER),
        ("version_2", patched(archive, 4, "<H", 2), BAD_HEADER),
        ("reserved_0", patched(archive, 24, "<I", 1), BAD_HEADER),
        ("reserved_1", patched(archive, 28, "<I", 0x80000000), BAD_HEADER),
        ("sections_0", patched(archive, 6, "<H", 0), BAD_COUNTS),
        ("sections_5", patched(archive, 6, "<H", 5), BAD_COUNTS),
        ("sections_other", patched(archive, 6, "<H", k % MAX_SECTIONS + 1), BAD_COUNTS),
        ("images_0", patched(archive, 8, "<I", 0), BAD_COUNTS),
        ("images_plus_1", patched(archive, 8, "<I", n + 1), BAD_COUNTS),
        ("images_huge", patched(archive, 8, "<I", 0xFFFFFFFF), BAD_COUNTS),
        ("size_huge", patched(archive, HEADER_BYTES + 4, "<I", 0xFFFFFFF0), BAD_SIZE),
        ("size_plus_16", patched(archive, HEADER_BYTES + 4, "<I", size1 + 16), BAD_TOTAL),
        ("size_zero", patched(archive, HEADER_BYTES + 4, "<I", 0), BAD_TOTAL),
        ("total_plus_16", patched(archive, 16, "<Q", total + 16), BAD_TOTAL),
        ("total_minus_16", patched(archive, 16, "<Q", total - 16), BAD_TOTAL),
        ("total_odd", patched(archive, 16, "<Q", total - 8), BAD_TOTAL),
        ("total_high_word", patched(archive, 20, "<I", 1), BAD_TOTAL),
        ("total_below_index", patched(archive, 16, "<Q", 32), BAD_TOTAL),
    ]
    return cases
