"""CPU-only checks of random access into a ragged archive (include/sicn_ragged_archive_select.h): the symbols and the binding table,
the host subset (sicn_ragged_archive_subset, codec.subset_archive) against the numpy statement of the format in
tests/archive_cases.py — the subset of an archive IS make_archive of the selected containers, byte for byte — every refusal, and
the argument checks of the device call that come before a device is asked for.  Nothing here touches a device."""
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
EINVAL, ENOSPC = -22, -28
U32P = ctypes.POINTER(ctypes.c_uint32)
FILL = 0xEE


def _declared_symbols():
    text = (ROOT / "include" / "sicn_ragged_archive_select.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicn_ragged_archive_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_select_symbol():
    L = _lib.lib()
    syms = _declared_symbols()
    assert syms == ["sicn_ragged_archive_subset", "sicn_ragged_archive_unpack_select_async"]
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_ARCHIVE_SELECT_ABI), "python binding table and sicn_ragged_archive_select.h disagree"
    assert not set(syms) & set(_lib.RAGGED_ARCHIVE_ABI)
    assert L.sicn_version() >= 11


def _subset(b: bytes, sel, capacity=None, out=True):
    """sicn_ragged_archive_subset with the output in a buffer of `capacity` bytes (default: the size a first call with out == NULL
    names) behind and in front of 32 guard bytes -> (rc, *out_bytes, what the buffer holds, guards untouched)."""
    L = _lib.lib()
    buf = (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(b.ljust(1, b"\0"))
    index = (ctypes.c_uint32 * max(len(sel), 1))(*sel)
    need = ctypes.c_uint64(12345)
    if not out:
        rc = L.sicn_ragged_archive_subset(buf, len(b), index, len(sel), None, 0, ctypes.byref(need))
        return rc, int(need.value), None, True
    if capacity is None:
        rc = L.sicn_ragged_archive_subset(buf, len(b), index, len(sel), None, 0, ctypes.byref(need))
        if rc:
            return rc, int(need.value), None, True
        capacity = int(need.value)
    whole = np.full(32 + capacity + 32, FILL, np.uint8)
    rc = L.sicn_ragged_archive_subset(buf, len(b), index, len(sel), ctypes.c_void_p(whole.ctypes.data + 32), capacity, ctypes.byref(need))
    return rc, int(need.value), whole[32:32 + capacity].tobytes(), bool((whole[:32] == FILL).all() and (whole[32 + capacity:] == FILL).all())


def _selections(n):
    return {"first": [0], "last": [n - 1], "all": list(range(n)), "every_other": list(range(0, n, 2)), "single": [n // 2]}


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 3, 257])
def test_subset_is_the_numpy_archive_of_the_selected_containers(n, k):
    """sample_containers' sizes walk around the 16-byte steps and include 0, so empty containers fall inside and outside every
    selection but the smallest."""
    containers = ac.sample_containers(n, k, seed=100 * n + k)
    tag = 0xB0000000 + n
    b = ac.make_archive(containers, tag)
    rows = codec.split_archive(b)
    for name, sel in _selections(n).items():
        want = ac.make_archive([containers[i] for i in sel], tag)
        rc, need, got, guards = _subset(b, sel)
        assert rc == 0 and need == len(want) and guards, name
        assert got == want, f"{name}: differs at byte {next(i for i in range(len(want)) if got[i] != want[i])}"
        assert _subset(b, sel, out=False)[:2] == (0, len(want)), name
        assert codec.subset_archive(b, sel) == want, name
        info = _lib.RaggedArchiveInfo()
        assert _lib.lib().sicn_ragged_archive_parse(got, len(got), ctypes.byref(info), None, None) == 0, name
        assert (info.n_images, info.n_sections, info.tag, info.total_bytes) == (len(sel), k, tag, len(want))
        assert codec.split_archive(got) == [rows[i] for i in sel], name
        # one byte short: SICN_ENOSPC, the size needed, and nothing written
        rc, need, held, guards = _subset(b, sel, capacity=len(want) - 1)
        assert (rc, need) == (ENOSPC, len(want)) and guards and held == bytes([FILL]) * (len(want) - 1), name


def test_empty_containers_inside_and_outside_the_selection():
    sizes = [[0, 0], [17, 0], [0, 0], [0, 33], [16, 16], [0, 0]]
    containers = ac.sample_containers(6, 2, seed=8, sizes=sizes)
    b = ac.make_archive(containers, 3)
    for sel in ([0], [2, 5], [0, 2, 5], [1, 3], [0, 1], [4], [3, 4, 5]):
        assert codec.subset_archive(b, sel) == ac.make_archive([containers[i] for i in sel], 3), sel
    assert len(codec.subset_archive(b, [0, 2, 5])) == 32 + 32                    # a header and an index, no payload


def test_every_refusal_of_subset_is_einval():
    n, k = 4, 2
    good = ac.make_archive(ac.sample_containers(n, k, seed=5, sizes=[[17, 40], [0, 16], [1, 33], [5, 0]]), tag=9)
    assert _subset(good, [1, 3])[0] == 0
    for name, bad, bit in ac.hostile(good, n, k):
        rc, need, _, _ = _subset(bad, [1, 3], out=False)
        assert (rc, need) == (EINVAL, 0), name
        rc, need, held, guards = _subset(bad, [1, 3], capacity=len(good))
        assert (rc, need) == (EINVAL, 0) and guards and held == bytes([FILL]) * len(good), name
        with pytest.raises(_lib.SicnError):
            codec.subset_archive(bad, [1, 3])
    small = ac.make_archive(ac.sample_containers(3, 2, seed=3), tag=1)
    for length in range(len(small)):
        assert _subset(small[:length], [0, 2], out=False)[0] == EINVAL, length
    assert _subset(small + b"bytes behind total_bytes are not the archive's", [0, 2])[2] == _subset(small, [0, 2])[2]
    # the selection
    for sel in ([n], [0, n], [0xFFFFFFFF], [1, 1], [0, 2, 2], [2, 1], [0, 3, 1], [3, 2, 1, 0], [0, 1, 2, 3, 3]):
        assert _subset(good, sel, out=False)[:2] == (EINVAL, 0), sel
        rc, _, held, guards = _subset(good, sel, capacity=len(good))
        assert rc == EINVAL and guards and held == bytes([FILL]) * len(good), sel
    assert _subset(good, [], out=False)[0] == EINVAL                              # n_selected == 0
    for sel in ([1, 1], [2, 1], [], [-1]):
        with pytest.raises(ValueError):
            codec.subset_archive(good, sel)
    with pytest.raises(_lib.SicnError):                                           # only the library knows the archive's n_images
        codec.subset_archive(good, [n])
    # NULLs
    L = _lib.lib()
    buf = (ctypes.c_uint8 * len(good)).from_buffer_copy(good)
    index = (ctypes.c_uint32 * 2)(1, 3)
    need = ctypes.c_uint64()
    assert L.sicn_ragged_archive_subset(buf, len(good), index, 2, None, 0, ctypes.byref(need)) == 0
    assert L.sicn_ragged_archive_subset(None, len(good), index, 2, None, 0, ctypes.byref(need)) == EINVAL
    assert L.sicn_ragged_archive_subset(buf, len(good), None, 2, None, 0, ctypes.byref(need)) == EINVAL
    assert L.sicn_ragged_archive_subset(buf, len(good), index, 2, None, 0, None) == EINVAL


def test_select_call_rejects_bad_arguments_without_a_device():
    L = _lib.lib()
    dummy = ctypes.c_void_p(64)
    four = (ctypes.c_void_p * 4)(64, 64, 64, 64)
    call = L.sicn_ragged_archive_unpack_select_async
    assert call(None, dummy, 1 << 20, 0, dummy, four, four, dummy, dummy, 1 << 20, None) == EINVAL           # a NULL object
    assert call(None, dummy, 1 << 20, 0, None, four, four, dummy, dummy, 1 << 20, None) == EINVAL            # a NULL index
    for odd in (65, 66, 67):
        assert call(None, dummy, 1 << 20, 0, ctypes.c_void_p(odd), four, four, dummy, dummy, 1 << 20, None) == EINVAL
    # with an object (where a gfx950 device exists to create one): the index is looked at before anything is enqueued
    u64p = ctypes.POINTER(ctypes.c_uint64)
    off, cap = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(64)
    h = ctypes.c_void_p()
    rc = L.sicn_ragged_archive_create(1, 1, (u64p * 1)(ctypes.cast(off, u64p)), (u64p * 1)(ctypes.cast(cap, u64p)), ctypes.byref(h))
    assert rc in (0, -19)
    if rc == 0:
        assert call(h, dummy, 1 << 20, 0, None, four, four, dummy, dummy, 1 << 20, None) == EINVAL
        assert call(h, dummy, 1 << 20, 0, ctypes.c_void_p(66), four, four, dummy, dummy, 1 << 20, None) == EINVAL
        L.sicn_ragged_archive_free(h)


def test_host_subset_under_the_sanitizers(tmp_path):
    """tests/cpp/archive_subset_check.cpp — the pure-host header with its own main — built with the address and undefined-behaviour
    sanitizers and run as a child process: every source archive and every output in a heap block of exactly its length, hostile
    archives, hostile selections and a capacity one byte short."""
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "archive_subset_check"
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([gxx, *flags, str(ROOT / "tests" / "cpp" / "archive_subset_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|unrecognized.*-fsanitize", r.stderr):
        pytest.skip(f"the compiler cannot link the sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0 and "ASan runtime does not come first in initial library list" in r.stderr:
        pytest.skip("a library preloaded into every process here comes before the sanitizer's runtime, which refuses to start behind it")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"archive_subset_check ok: \d+ checks", r.stdout), r.stdout
