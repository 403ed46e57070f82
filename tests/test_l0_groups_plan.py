"""The channel groups of layer 0 in the live-channel plan (csrc/sicn_live.h) without a GPU: tests/cpp/call_plan_check.cpp is the
plan header and nothing else, compiled here with -fsanitize=address,undefined and run on weight sets written to a temporary directory.
A 3 -> 128 layer without a GDN whose consumer reads at most 96 of its channels computes and stores three of the four 32-channel
groups: the live channels go, ascending, to the positions 0, 1, 2, ..., the dead ones behind them, and the consumer's K index moves
with them.  What the program says about the tables, about one call's walk (the groups that run, the groups behind a layer's input, the
copy of the weights a layer takes: 0 = the caller's own handle) and about the permuted copies is held to the reference's PARAM tables and
to numpy statements of the same permutation.  As in tests/test_live_plan.py the device images are not packed here: a derived handle is
the ordinary packers' output on the permuted w_okc checked below (weights_from_okc, csrc/sicn_abi.hip)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import sicn_ref

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "call_plan_check.cpp"
GOLDEN = ROOT / "tests" / "golden" / "param_weights.npz"
# (cin, cout, gdn, planned onto the wide family, layout towards the next layer: 1 = GROUP, 2 = PHASE, transposed, on the layer-7 family)
# of the reference's eight layers on a large input
NET = [(3, 128, 0, 0, 1, 0, 0), (128, 128, 0, 1, 1, 0, 0), (128, 128, 0, 1, 1, 0, 0), (128, 192, 0, 0, 1, 0, 0), (192, 128, 0, 0, 2, 1, 0),
       (128, 128, 0, 1, 2, 1, 0), (128, 128, 0, 1, 2, 1, 0), (128, 3, 0, 0, 0, 1, 1)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    out = tmp_path_factory.mktemp("l0_groups_plan") / "call_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", str(SRC), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def _param(n=8):
    return [(w.reshape(w.shape[0], -1).astype(np.int8), b.astype(np.int8)) for w, b, _ in sicn_ref.load_param_fixture(GOLDEN)][:n]


def _random(seed, n_dead, n=3):
    """layers 0 .. n - 1 with dense random weights, n_dead random input channels of layer 1 zero in every tap"""
    rng = np.random.default_rng(seed)
    net = []
    for l, (cin, cout, *_) in enumerate(NET[:n]):
        w = rng.integers(-8, 8, (cout, 25, cin)).astype(np.int8)
        if l == 1 and n_dead:
            w[:, :, rng.permutation(128)[:n_dead]] = 0
        net.append((w.reshape(cout, -1), rng.integers(-128, 128, cout).astype(np.int8)))
    return net


def _run(exe, d, weights, first=0, last=None, tap=-1, meta=NET):
    n = len(weights)
    last = n - 1 if last is None else last
    for l, (w, b) in enumerate(weights):
        w.tofile(d / f"l{l}.okc")
        b.tofile(d / f"l{l}.bias")
    (d / "meta.txt").write_text("".join(" ".join(map(str, m)) + "\n" for m in meta[:n]))
    r = subprocess.run([str(exe), str(d), str(n), str(first), str(last), str(tap)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr     # a sanitizer report ends the program with an error
    rows, perm = {}, {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "L":
            rows[int(f[1])] = {f[i]: int(f[i + 1]) for i in range(2, len(f), 2)}
        elif f[0] == "G":
            perm[int(f[1])] = [int(v) for v in f[2:]]
    return [rows[l] for l in range(n)], perm


def _check_images(d, weights, p):
    """p (layer 0's) is a permutation, live channels ascending at 0, 1, 2, ..., dead ones ascending behind; the copies are numpy's"""
    p = np.array(p)
    assert sorted(p.tolist()) == list(range(128))
    w1 = weights[1][0].reshape(weights[1][0].shape[0], 25, 128)
    alive = np.flatnonzero(np.any(w1 != 0, axis=(0, 1)))
    dead = np.setdiff1d(np.arange(128), alive)
    assert p[alive].tolist() == list(range(len(alive))), "the live channels sit at 0 .. n - 1 in ascending order"
    assert p[dead].tolist() == list(range(len(alive), 128))
    assert len(alive) <= 96
    w, b = weights[0]
    w_out, b_out = np.empty_like(w), np.empty_like(b)
    w_out[p], b_out[p] = w, b
    assert np.array_equal(np.fromfile(d / "l0.out.okc", np.int8).reshape(w.shape), w_out)
    assert np.array_equal(np.fromfile(d / "l0.out.bias", np.int8), b_out)
    k_in = np.empty_like(w1)
    k_in[:, :, p] = w1
    got = np.fromfile(d / "l1.in.okc", np.int8).reshape(w1.shape)
    assert np.array_equal(got, k_in)
    assert not np.any(got[:, :, len(alive):]), "layer 1's input-permuted image is zero behind the live positions in every tap"
    assert not np.any(got[:, :, 96:]), "and so in the whole fourth group"
    return len(alive)


def test_param_tables(exe, tmp_path):
    weights = _param()
    rows, perm = _run(exe, tmp_path, weights, 0, 7, 3)
    assert rows[0] == {"live": 80, "nj": 8, "ng": 3, "groups": 3, "groups_in": 4, "variant": 1, "halves": 2, "walk": 4}, rows[0]
    assert rows[1] == {"live": 80, "nj": 5, "ng": 4, "groups": 4, "groups_in": 3, "variant": 3, "halves": 2, "walk": 3}, rows[1]
    assert [r["walk"] for r in rows[2:]] == [4] * 6 and [r["halves"] for r in rows] == [2] * 7 + [1]
    assert [r["groups"] for r in rows[1:]] == [4] * 7 and [r["groups_in"] for r in rows[2:]] == [4] * 6
    assert [r["ng"] for r in rows[1:]] == [4] * 7
    assert [r["variant"] for r in rows] == [1, 3, 3, 2, 0, 1, 3, 2]      # layers 1 .. 7 as before the groups
    assert [r["nj"] for r in rows] == [8, 5, 5, 8, 8, 5, 3, 8]
    assert sorted(perm) == [0]
    assert _check_images(tmp_path, weights, perm[0]) == 80
    assert perm[0][:8] == [0, 1, 2, 3, 4, 80, 81, 82]                    # c mod 8 >= 5 is dead


def test_param_calls_that_end_or_tap_at_layer_1(exe, tmp_path):
    """layer 0 runs 3 groups, layer 1 all 8 columns on the input-permuted copy alone"""
    for last, tap in ((1, -1), (2, 1)):
        rows, _ = _run(exe, tmp_path, _param(3), 0, last, tap)
        assert (rows[0]["groups"], rows[0]["variant"]) == (3, 1)
        assert (rows[1]["nj"], rows[1]["groups_in"], rows[1]["variant"], rows[1]["walk"]) == (8, 3, 2, 3), rows[1]
        if last == 2:
            assert (rows[2]["groups_in"], rows[2]["variant"]) == (4, 0), rows[2]


@pytest.mark.parametrize("n_dead, groups", [(32, 3), (31, 4), (0, 4), (48, 3), (80, 3)])
def test_random_dead_sets(exe, tmp_path, n_dead, groups):
    weights = _random(100 + n_dead, n_dead)
    rows, perm = _run(exe, tmp_path, weights)
    assert (rows[0]["live"], rows[0]["ng"], rows[0]["groups"], rows[0]["nj"]) == (128 - n_dead, groups, groups, 8), rows[0]
    assert rows[1]["groups_in"] == groups and rows[0]["variant"] == int(groups == 3) and rows[1]["variant"] >> 1 == int(groups == 3)
    assert [r["walk"] for r in rows] == [4, groups, 4]
    assert sorted(perm) == ([0] if groups == 3 else [])
    if groups == 3:
        assert _check_images(tmp_path, weights, perm[0]) == 128 - n_dead


def test_calls_that_keep_four_groups_and_the_standard_handles(exe, tmp_path):
    weights = _param(3)
    # a GDN on layer 0: the activation mixes the channels, the table itself has 4 groups and no permutation
    meta = [list(m) for m in NET]
    meta[0][2] = 1
    rows, perm = _run(exe, tmp_path, weights, meta=meta)
    assert (rows[0]["ng"], rows[0]["groups"], rows[0]["variant"], rows[0]["live"]) == (4, 4, 0, 128) and 0 not in perm, rows[0]
    assert (rows[1]["groups_in"], rows[1]["variant"]) == (4, 1), rows[1]
    # a call [0, 0]: layer 0 is the call's last layer
    rows, _ = _run(exe, tmp_path, weights, 0, 0, -1)
    assert (rows[0]["ng"], rows[0]["groups"], rows[0]["variant"]) == (3, 4, 0), rows[0]
    # a tap at layer 0: its output leaves the chain, layer 1 reads it in its own order
    rows, _ = _run(exe, tmp_path, weights, 0, 2, 0)
    assert (rows[0]["groups"], rows[0]["variant"], rows[0]["live"]) == (4, 0, 128), rows[0]
    assert (rows[1]["groups_in"], rows[1]["variant"]) == (4, 1), rows[1]
    # a call that starts behind layer 0, and an output that does not leave in the GROUP layout
    rows, _ = _run(exe, tmp_path, weights, 1, 2, -1)
    assert (rows[0]["groups"], rows[1]["groups_in"], rows[1]["variant"]) == (4, 4, 1)
    meta = [list(m) for m in NET]
    meta[0][4] = 0
    rows, _ = _run(exe, tmp_path, weights, meta=meta)
    assert (rows[0]["ng"], rows[0]["groups"], rows[0]["variant"], rows[1]["groups_in"]) == (3, 4, 0, 4), rows[0]
    assert rows[1]["walk"] == 4
