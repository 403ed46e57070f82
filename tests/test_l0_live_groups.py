"""What keeps tests/test_l0_live_groups_gpu.py from hiding a failure, checked where no GPU is needed (the spirit of
tests/test_live_geometry.py).

Coverage of positions.  Layer 0 with three groups computes the positions 0 .. 95; a wrong byte at a position whose channel layer 1
multiplies by zero cannot fail anything.  tests/cpp/call_plan_check.cpp (the plan header alone, compiled with
-fsanitize=address,undefined) on the weight sets of the GPU file: with 32 dead channels the live ones fill ALL 96 computed positions,
with 48 (random and PARAM) the positions 0 .. 79, and every one of those is read; the controls keep four groups and no permutation.

Sensitivity.  The byte comparison behind layer 1 sees a wrong byte of layer 0 only if layer 1's output changes with it.  With the oracle
alone: one byte of layer 0's output changed by + 1 and by + 128 (mod 256), in every live channel, at the four corners of the map and on
both sides of every edge of k_l0's first tile; every single trial must change layer 1's output.  A trial runs layer 1 on a window of the
map that holds the +- 4 neighbourhood of the byte (cut only where the map ends, its origin even so that the stride-2 phase stays): the
outputs that the byte reaches are the map's own there, every other output is the same with and without the change.  A few trials are
run on the whole map as well and must count the same changed bytes."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import l0_groups_cases as gc
from oracle import c_oracle
from simple_image_compression_network_amd.config import LayerDesc

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "call_plan_check.cpp"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    out = tmp_path_factory.mktemp("l0_live_groups") / "call_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", str(SRC), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.mark.parametrize("wset", list(gc.SETS))
def test_live_channels_fill_the_computed_positions_from_zero(exe, tmp_path, wset):
    for l in range(3):
        w, b = gc.weights(wset, l)
        gc.okc(w).tofile(tmp_path / f"l{l}.okc")
        b.tofile(tmp_path / f"l{l}.bias")
    (tmp_path / "meta.txt").write_text("3 128 0 0 1 0 0\n128 128 0 1 1 0 0\n128 128 0 1 1 0 0\n")
    r = subprocess.run([str(exe), str(tmp_path), "3", "0", "2", "-1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr     # a sanitizer report ends the program with an error
    lines = [ln.split() for ln in r.stdout.splitlines()]
    row0 = next(f for f in lines if f[:2] == ["L", "0"])
    perm = [[int(v) for v in f[2:]] for f in lines if f[:2] == ["G", "0"]]
    n_live = 128 - gc.SETS[wset]
    alive = gc.live_channels(gc.weights(wset, 1)[0])
    assert len(alive) == n_live and int(row0[row0.index("live") + 1]) == n_live
    assert int(row0[row0.index("groups") + 1]) == gc.groups(wset)
    if gc.groups(wset) == 4:
        assert not perm
        return
    assert {perm[0][c] for c in alive} == set(range(n_live)), "computed positions below the live count that layer 1 does not read"
    assert n_live == 96 or wset in ("param", "r48")


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
W, H = 260, 136                              # the GPU file's ragged geometry: layer 0 writes 130 x 68
REACH = 4


def _positions(h, w):
    th, tw = gc.L0_TILE_H, gc.L0_TILE_W
    assert th < h and tw < w
    return [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (th - 1, tw - 1), (0, tw), (th, 0), (th - 1, tw), (th, tw - 1)]


def _layer1(wd, b, x):
    d = LayerDesc.make(128, 128, 8, 16, x.shape[1], x.shape[0], 0)
    return c_oracle.run_layer(d, wd, b, x, form="direct", threads=1)


@pytest.mark.parametrize("wset", ["param", "r48", "r32"])
def test_every_wrong_live_byte_changes_layer_1(wset):
    y = gc.reference(wset, W, H, 1, 1)[0][0]
    mh, mw = y.shape[:2]
    assert (mw, mh) == (130, 68)
    wt, b = gc.weights(wset, 1)
    wd = gc.words(1, wt)
    alive = gc.live_channels(wt)
    trials, undetected, whole_map, full = 0, [], 0, None
    for (py, px) in _positions(mh, mw):
        y0, x0 = max(0, (py - REACH) & ~1), max(0, (px - REACH) & ~1)
        win = np.ascontiguousarray(y[y0:min(mh, py + REACH + 1), x0:min(mw, px + REACH + 1)])
        base = _layer1(wd, b, win)
        for c in alive:
            for delta in (1, 128):
                t = win.copy()
                t[py - y0, px - x0, c] = (int(t[py - y0, px - x0, c]) + delta) & 0xFF
                changed = int(np.count_nonzero(_layer1(wd, b, t) != base))
                trials += 1
                if not changed:
                    undetected.append((py, px, int(c), delta))
                if trials % 97 == 0:                 # the same trial on the whole map: the window tells the truth
                    full = _layer1(wd, b, y) if full is None else full
                    t = y.copy()
                    t[py, px, c] = (int(t[py, px, c]) + delta) & 0xFF
                    assert int(np.count_nonzero(_layer1(wd, b, t) != full)) == changed, (py, px, int(c), delta)
                    whole_map += 1
    assert trials == 9 * 2 * len(alive) and len(alive) == 128 - gc.SETS[wset] and whole_map >= 14
    if wset == "param":
        # the PARAM tables are no test vectors: behind their ReLU 49 of the 1440 single-byte changes are invisible (at the corners,
        # where few outputs see the byte).  What must hold of them is that no live CHANNEL is invisible; byte by byte the random sets
        # are the ones that catch a fault, below
        print(f"param: {len(undetected)} of {trials} single wrong bytes left layer 1's output unchanged")
        blind = [int(c) for c in alive if sum(1 for u in undetected if u[2] == c) == 18]     # 9 positions x 2 changes
        assert not blind, f"live channels whose bytes no trial saw: {blind}"
        return
    assert not undetected, f"{len(undetected)} of {trials} wrong bytes left layer 1's output unchanged: {undetected[:8]}"
