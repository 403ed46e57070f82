"""What keeps tests/test_live_geometry_gpu.py from hiding a failure, checked where no GPU is needed.

Coverage of positions.  A live kernel with NJ columns computes the positions of the columns 0 .. NJ - 1 (16 NJ of 128); a wrong byte at
a position whose channel the consumer multiplies by zero cannot fail anything.  tests/cpp/call_plan_check.cpp (the plan header alone,
compiled with -fsanitize=address,undefined as tests/test_live_plan.py does) on the weight sets of the GPU file: with 80 dead channels the
live ones fill ALL 48 positions of 3 columns, with 48 dead all 80 of 5 columns - and with 112 dead, the only 3-column case with random
weights that the suite had, 16 of the 48.

Sensitivity.  The byte comparison behind a consumer sees a wrong producer byte only if the consumer's output changes with it.  With the
oracle alone: one byte of the producer's output changed by + 1 and by + 128 (mod 256), in every live channel, at the four corners of
the map and on both sides of every edge of the first tile, for every kind of consumer at the two odd geometries; every single trial must
change the consumer's output.  A trial runs the consumer on a window of the map: a changed byte at (y, x) reaches only outputs whose
5 x 5 taps cover it, and all inputs of those outputs lie within +- 4 positions of (y, x), so on a window that holds that
neighbourhood (cut only where the map itself ends, its origin even so that the stride-2 phases stay) those outputs are the map's own
bytes, and every other output is the same with and without the change.  A few trials are run on the whole map as well and must count
the same changed bytes."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import live_geometry_cases as lg
from oracle import c_oracle

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "call_plan_check.cpp"
SEED = 20                                    # tests/test_live_geometry_gpu.py
CHAINS = [("conv", "conv"), ("deconv", "rgb"), ("deconv", "deconv"), ("conv", "conv", "conv192"), ("deconv", "deconv", "rgb")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    out = tmp_path_factory.mktemp("live_geometry") / "call_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", str(SRC), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def _plan(exe, d, kinds, wts):
    """(live outputs, columns, permutation) per layer of a call over the whole chain, no tap"""
    for l, (w, b) in enumerate(wts):
        lg.okc(w).tofile(d / f"l{l}.okc")
        b.tofile(d / f"l{l}.bias")
    (d / "meta.txt").write_text("".join(f"128 {lg.KINDS[k][0]} 0 {int(k in ('conv', 'deconv'))} {2 if lg.KINDS[k][3] else 1} {lg.KINDS[k][3]} {int(k == 'rgb')}\n"
                                          for k in kinds))
    r = subprocess.run([str(exe), str(d), str(len(kinds)), "0", str(len(kinds) - 1), "-1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr     # a sanitizer report ends the program with an error
    live, nj, perm = {}, {}, {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "L":
            live[int(f[1])], nj[int(f[1])] = int(f[3]), int(f[5])
        elif f[0] == "P":
            perm[int(f[1])] = [int(v) for v in f[2:]]
    return live, nj, perm


def _column(pos):
    return 4 * (pos >> 6) + ((pos >> 2) & 3)     # csrc/k_mfma16x.hip: column j = 4 J + d holds positions 64 J + 16 g + 4 d + r


@pytest.mark.parametrize("cols", [3, 5])
@pytest.mark.parametrize("kinds", CHAINS, ids="-".join)
def test_live_channels_fill_every_computed_position(exe, tmp_path, kinds, cols):
    n_dead = lg.N_DEAD[cols]
    wts = lg.chain_weights(kinds, SEED, n_dead)
    live, nj, perm = _plan(exe, tmp_path, kinds, wts)
    last = len(kinds) - 1
    assert [nj[l] for l in range(last + 1)] == [cols] * last + [8] and [live[l] for l in range(last)] == [128 - n_dead] * last, (live, nj)
    assert sorted(perm) == list(range(last))
    computed = {pos for pos in range(128) if _column(pos) < cols}
    assert len(computed) == 16 * cols == 128 - n_dead
    for l in range(last):
        alive = lg.live_channels(wts[l + 1][0])
        assert len(alive) == 128 - n_dead
        assert {perm[l][c] for c in alive} == computed, f"layer {l}: computed positions that no consumer reads"


@pytest.mark.parametrize("kinds", [("conv", "conv"), ("deconv", "rgb")], ids="-".join)
def test_with_112_dead_channels_a_third_of_the_computed_positions_is_read(exe, tmp_path, kinds):
    """why this file exists: 16 live channels sit at the positions 0 .. 11 and 16 .. 19 (row group 0 of the columns 0, 1, 2, row group 1
    of column 0); the other 32 positions of a 3-column kernel are computed, stored and met by zero weights"""
    wts = lg.chain_weights(kinds, SEED, 112)
    live, nj, perm = _plan(exe, tmp_path, kinds, wts)
    assert (live[0], nj[0]) == (16, 3)
    assert {perm[0][c] for c in lg.live_channels(wts[1][0])} == set(range(12)) | set(range(16, 20))


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
SENSITIVITY = [("conv", 129, 67, "conv"), ("conv", 129, 67, "conv192"), ("deconv", 33, 17, "rgb"), ("deconv", 33, 17, "deconv")]
REACH = 4


def _positions(prod):
    """(y, x) in the producer's output: the four corners, and the last position of the first tile with the first positions of the tiles
    right of it and below it (a deconv tile of 16 x 32 inputs is 32 x 64 outputs)"""
    h, w = prod.OFM_COL, prod.OFM_ROW
    th, tw = (2 * lg.TILE_H, 2 * lg.TILE_W) if prod.transposed else (lg.TILE_H, lg.TILE_W)
    assert th < h and tw < w
    return [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (th - 1, tw - 1), (0, tw), (th, 0), (th - 1, tw), (th, tw - 1)]


def _run(kind, wd, b, x):
    return c_oracle.run_layer(lg.desc(kind, x.shape[1], x.shape[0]), wd, b, x, form="direct", threads=1)


@pytest.mark.parametrize("prod, w, h, cons", SENSITIVITY, ids=[f"{p}{w}x{h}-{c}" for p, w, h, c in SENSITIVITY])
def test_every_wrong_live_byte_changes_the_consumers_output(prod, w, h, cons):
    pd = lg.desc(prod, w, h)
    y = lg.reference((prod,), w, h, 1, SEED, 0)[0][0]
    mh, mw = y.shape[:2]
    trials, undetected, whole_map = 0, [], 0
    for cols in (3, 5):
        wt, b = lg.chain_weights((prod, cons), SEED, lg.N_DEAD[cols])[1]
        wd = lg.words(cons, wt)
        full = None
        for (py, px) in _positions(pd):
            y0, x0 = max(0, (py - REACH) & ~1), max(0, (px - REACH) & ~1)
            win = np.ascontiguousarray(y[y0:min(mh, py + REACH + 1), x0:min(mw, px + REACH + 1)])
            base = _run(cons, wd, b, win)
            for c in lg.live_channels(wt):
                for delta in (1, 128):
                    t = win.copy()
                    t[py - y0, px - x0, c] = (int(t[py - y0, px - x0, c]) + delta) & 0xFF
                    changed = int(np.count_nonzero(_run(cons, wd, b, t) != base))
                    trials += 1
                    if not changed:
                        undetected.append((cols, py, px, int(c), delta))
                    if trials % 97 == 0:                 # the same trial on the whole map: the window tells the truth
                        full = _run(cons, wd, b, y) if full is None else full
                        t = y.copy()
                        t[py, px, c] = (int(t[py, px, c]) + delta) & 0xFF
                        assert int(np.count_nonzero(_run(cons, wd, b, t) != full)) == changed, (cols, py, px, int(c), delta)
                        whole_map += 1
    assert trials == 9 * 2 * (48 + 80) and whole_map >= 20
    assert not undetected, f"{len(undetected)} of {trials} wrong bytes left the consumer's output unchanged: {undetected[:8]}"
