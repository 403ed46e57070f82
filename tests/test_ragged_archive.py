"""CPU-only checks of the ragged archive's ABI (include/sicn_ragged_archive.h): the symbols, the binding table, the format's arithmetic
(sicn_ragged_archive_layout) and the host parser (sicn_ragged_archive_parse) against the numpy statement of the format in
tests/archive_cases.py, and the argument checks of the object.  Nothing here touches a device."""
import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simple_image_compression_network_amd import _lib, codec
import archive_cases as ac

ROOT = Path(__file__).resolve().parent.parent
EINVAL = -22
U32P, U64P = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)


def _declared_symbols():
    text = (ROOT / "include" / "sicn_ragged_archive.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicn_ragged_archive_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_archive_symbol():
    L = _lib.lib()
    syms = _declared_symbols()
    assert len(syms) == 9
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_ARCHIVE_ABI), "python binding table and sicn_ragged_archive.h disagree"
    assert L.sicn_version() >= 10
    assert ctypes.sizeof(_lib.RaggedArchiveStatus) == 16 and ctypes.sizeof(_lib.RaggedArchiveInfo) == 32
    chunk = L.sicn_ragged_archive_chunk_bytes()
    assert chunk >= 16 and chunk % 16 == 0


def _layout(sizes, n, k, want_offsets=True):
    flat = np.ascontiguousarray(sizes, dtype=np.uint32).reshape(-1)
    offsets = (ctypes.c_uint64 * max(flat.size, 1))()
    total = ctypes.c_uint64(0)
    rc = _lib.lib().sicn_ragged_archive_layout(flat.ctypes.data_as(U32P), n, k, offsets if want_offsets else None, ctypes.byref(total))
    return rc, [int(v) for v in offsets[:flat.size]], int(total.value)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_layout_equals_plain_arithmetic_around_the_16_byte_steps(k):
    steps = [0, 1, 15, 16, 17, 31, 32, 33, 0, 4096, 16383, 16384, 16385]
    for n in (1, 2, 3, 4, 5, 7, 13):                      # index paddings of 0, 4, 8 and 12 bytes occur for every k
        sizes = [[steps[(i * k + s) % len(steps)] for s in range(k)] for i in range(n)]
        rc, offsets, total = _layout(sizes, n, k)
        want_offsets, want_total = ac.layout(sizes)
        assert rc == 0 and offsets == want_offsets and total == want_total
        assert total % 16 == 0 and all(o % 16 == 0 for o in offsets)
        assert offsets[0] == 32 + ac.a16(4 * n * k)
        assert _layout(sizes, n, k, want_offsets=False)[2] == total


def test_index_padding_takes_every_value():
    seen = set()
    for n, k in [(4, 1), (1, 4), (2, 2), (3, 1), (1, 3), (1, 2), (2, 1), (3, 2), (1, 1), (5, 1), (7, 1)]:
        rc, offsets, _ = _layout(np.ones((n, k)), n, k)
        assert rc == 0
        pad = offsets[0] - 32 - 4 * n * k
        assert pad == -(4 * n * k) % 16
        seen.add(pad)
    assert seen == {0, 4, 8, 12}


def test_offsets_are_64_bit():
    """A payload that passes 2^32: 3 images x 2 sections of almost 4 GiB each — arithmetic only, nothing is allocated."""
    sizes = [[0xFFFFFFFF, 0xFFFFFFF1], [1, 0xFFFFFFF0], [0, 17]]
    rc, offsets, total = _layout(sizes, 3, 2)
    assert rc == 0
    assert (offsets, total) == ac.layout(sizes)
    assert offsets[2] == 32 + 32 + 2 * 2 ** 32 and total > 3 * 2 ** 32


def test_layout_limits_are_einval():
    L = _lib.lib()
    one = np.ones(8, np.uint32).ctypes.data_as(U32P)
    total = ctypes.c_uint64()
    assert L.sicn_ragged_archive_layout(one, 2, 4, None, ctypes.byref(total)) == 0
    assert L.sicn_ragged_archive_layout(one, 2, 4, None, None) == 0                    # both outputs are optional
    assert L.sicn_ragged_archive_layout(one, 0, 1, None, ctypes.byref(total)) == EINVAL
    assert L.sicn_ragged_archive_layout(one, 1, 0, None, ctypes.byref(total)) == EINVAL
    assert L.sicn_ragged_archive_layout(one, 1, 5, None, ctypes.byref(total)) == EINVAL
    assert L.sicn_ragged_archive_layout(None, 1, 1, None, ctypes.byref(total)) == EINVAL
    assert L.sicn_ragged_archive_layout(one, 2 ** 24 + 1, 1, None, ctypes.byref(total)) == EINVAL
    assert L.sicn_ragged_archive_layout(one, 2 ** 23 + 1, 2, None, ctypes.byref(total)) == EINVAL
    big = np.zeros(2 ** 24, np.uint32)
    assert L.sicn_ragged_archive_layout(big.ctypes.data_as(U32P), 2 ** 24, 1, None, ctypes.byref(total)) == 0
    assert total.value == 32 + 4 * 2 ** 24


def _parse(b: bytes, want=True):
    L = _lib.lib()
    buf = (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(b.ljust(1, b"\0"))
    info = _lib.RaggedArchiveInfo()
    rc = L.sicn_ragged_archive_parse(buf, len(b), ctypes.byref(info), None, None)
    if rc or not want:
        return rc, info, None, None
    entries = info.n_images * info.n_sections
    sizes, offsets = (ctypes.c_uint32 * entries)(), (ctypes.c_uint64 * entries)()
    rc = L.sicn_ragged_archive_parse(buf, len(b), ctypes.byref(info), sizes, offsets)
    return rc, info, list(sizes), list(offsets)


@pytest.mark.parametrize("n,k", [(1, 1), (5, 1), (3, 2), (2, 3), (4, 4), (7, 1), (300, 2)])
def test_parse_returns_what_numpy_wrote(n, k):
    containers = ac.sample_containers(n, k, seed=n * 10 + k)
    b = ac.make_archive(containers, tag=0xA5A50000 + n)
    rc, info, sizes, offsets = _parse(b)
    assert rc == 0
    want_sizes = [len(c) for cs in containers for c in cs]
    want_offsets, total = ac.layout(np.asarray(want_sizes).reshape(n, k))
    assert total == len(b)
    assert (info.version, info.n_sections, info.n_images, info.tag, info.total_bytes) == (1, k, n, 0xA5A50000 + n, total)
    assert info.payload_offset == 32 + ac.a16(4 * n * k)
    assert sizes == want_sizes and offsets == want_offsets
    assert codec.split_archive(b) == containers
    assert codec.split_archive(b + b"bytes behind total_bytes are not the archive's") == containers


def test_every_rejection_is_einval_each_from_one_patched_field():
    n, k = 4, 2
    good = ac.make_archive(ac.sample_containers(n, k, seed=5, sizes=[[17, 40], [0, 16], [1, 33], [5, 0]]), tag=9)
    assert _parse(good)[0] == 0
    cases = ac.hostile(good, n, k)
    assert {bit for _, _, bit in cases} == {ac.BAD_HEADER, ac.BAD_COUNTS, ac.BAD_SIZE, ac.BAD_TOTAL}
    for name, bad, _ in cases:
        assert bad != good, name
        assert _parse(bad)[0] == EINVAL, name
        with pytest.raises(_lib.SicnError):
            codec.split_archive(bad)
    # the index's padding is part of the format (6 entries: 8 bytes of it)
    padded = ac.make_archive(ac.sample_containers(3, 2, seed=5, sizes=[[17, 40], [0, 16], [1, 33]]), tag=9)
    assert _parse(padded)[0] == 0
    assert _parse(ac.patched(padded, 32 + 24, "<B", 1))[0] == EINVAL
    assert _parse(ac.patched(padded, 32 + 31, "<B", 0x80))[0] == EINVAL
    # the tag is opaque to the host parser
    rc, info, _, _ = _parse(ac.patched(good, 12, "<I", 0xDEADBEEF))
    assert rc == 0 and info.tag == 0xDEADBEEF
    L = _lib.lib()
    info = _lib.RaggedArchiveInfo()
    assert L.sicn_ragged_archive_parse(None, 64, ctypes.byref(info), None, None) == EINVAL
    buf = (ctypes.c_uint8 * len(good)).from_buffer_copy(good)
    assert L.sicn_ragged_archive_parse(buf, len(good), None, None, None) == EINVAL


def test_a_valid_archive_truncated_to_every_length_is_einval():
    good = ac.make_archive(ac.sample_containers(4, 2, seed=3), tag=1)
    assert _parse(good)[0] == 0
    for length in range(len(good)):
        assert _parse(good[:length], want=False)[0] == EINVAL, length


def _create(off, cap, n=None, k=None, out=True):
    """sicn_ragged_archive_create with slot_offset / slot_bytes given as [k][n] lists (None: a null section pointer)."""
    L = _lib.lib()
    k = len(off) if k is None else k
    n = len(off[0]) if n is None else n
    keep = []

    def table(rows):
        if rows is None:
            return None
        arr = (U64P * max(len(rows), 1))()
        for s, r in enumerate(rows):
            if r is not None:
                a = (ctypes.c_uint64 * max(len(r), 1))(*r)
                keep.append(a)
                arr[s] = ctypes.cast(a, U64P)
        return arr
    h = ctypes.c_void_p()
    rc = L.sicn_ragged_archive_create(n, k, table(off), table(cap), ctypes.byref(h) if out else None)
    return rc, h


def test_every_einval_of_create():
    """Every argument check comes before the device is asked for, so these hold without one; a well-formed call gets past them (and
    then succeeds, or answers SICN_ENODEV where there is no gfx950 device)."""
    L = _lib.lib()
    rc, h = _create([[0, 64]], [[64, 64]])
    assert rc in (0, -19)
    if rc == 0:
        assert L.sicn_ragged_archive_workspace_bytes(h) >= 12 * 2 and L.sicn_ragged_archive_max_bytes(h) == 32 + 16 + 128
        L.sicn_ragged_archive_free(h)
    per_slot = -(-(2 ** 32 - 1) // L.sicn_ragged_archive_chunk_bytes())          # work items of one slot just below 4 GiB
    many = -(-(2 ** 31 - 1) // per_slot)
    bad = [
        _create([[0]], [[64]], n=0),                                   # n_images < 1
        _create([[0]], [[64]], n=-1),
        _create([[0]], [[64]], k=0),                                   # n_sections outside 1 .. 4
        _create([[0]] * 5, [[64]] * 5),
        _create([[0]], [[64]], n=2 ** 24 + 1),                         # n_images * n_sections > 2^24 (refused before a table is read)
        _create([[0]] * 2, [[64]] * 2, n=2 ** 23 + 1),
        _create([[0, 64]], [[64, 2 ** 32]]),                           # a slot of 4 GiB or more
        _create([[0, 64]], [[2 ** 40, 64]]),
        _create([[0, 72]], [[64, 64]]),                                # a slot offset that is not a multiple of 16
        _create([[1, 64]], [[64, 64]]),
        _create([[0], [8]], [[64], [64]]),
        _create([[i << 32 for i in range(many)]], [[2 ** 32 - 1] * many]),   # 2^31 - 1 work items or more (8192 slots of 2^18 chunks at 16 KiB)
        _create(None, [[64]], n=1, k=1),                               # a null pointer
        _create([[0]], None, n=1, k=1),
        _create([[0], None], [[64], [64]]),
        _create([[0], [0]], [[64], None]),
        _create([[0]], [[64]], out=False),
    ]
    for i, (rc, h) in enumerate(bad):
        assert rc == EINVAL and not h.value, i
    rc, h = _create([[0, 64]], [[64, 2 ** 32 - 1]])                     # one byte below 4 GiB is a slot like any other
    assert rc in (0, -19)
    if rc == 0:
        L.sicn_ragged_archive_free(h)
    assert L.sicn_ragged_archive_workspace_bytes(None) == 0 and L.sicn_ragged_archive_max_bytes(None) == 0
    L.sicn_ragged_archive_free(None)


def test_calls_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    dummy = ctypes.c_void_p(64)
    two = (ctypes.c_void_p * 4)(64, 64, 64, 64)
    assert L.sicn_ragged_archive_pack_async(None, two, two, 0, dummy, 1 << 20, dummy, dummy, 1 << 20, None) == EINVAL
    assert L.sicn_ragged_archive_unpack_async(None, dummy, 1 << 20, 0, two, two, dummy, dummy, 1 << 20, None) == EINVAL


def test_host_parser_under_the_sanitizers(tmp_path):
    """tests/cpp/archive_parse_check.cpp — the pure-host header with its own main — built with the address and undefined-behaviour
    sanitizers and run as a child process: the hostile and truncated archives again, every one in a heap block of exactly its length."""
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "archive_parse_check"
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([gxx, *flags, str(ROOT / "tests" / "cpp" / "archive_parse_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|unrecognized.*-fsanitize", r.stderr):
        pytest.skip(f"the compiler cannot link the sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0 and "ASan runtime does not come first in initial library list" in r.stderr:
        pytest.skip("a library preloaded into every process here comes before the sanitizer's runtime, which refuses to start behind it")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"archive_parse_check ok: \d+ checks", r.stdout), r.stdout
