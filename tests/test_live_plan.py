"""The live-channel plan (csrc/sicn_live.h) without a GPU: tests/cpp/call_plan_check.cpp is the plan header and nothing else, compiled
here with -fsanitize=address,undefined and run on weight sets written to a temporary directory.  What it says about a call is held to
the reference's PARAM tables and to numpy statements of the same permutation.
The device images themselves are not packed here.  The packers (pack_mfma16_stream, pack_mfma16x_deconv_stream, pack_l7, ...) live in
translation units with device code and have no stand-alone host build; a net hands them the permuted w_okc and bias checked below
through the one function that also serves sicn_weights_from_finn_tiles (weights_from_okc, csrc/sicn_abi.hip), so an image of a derived
handle IS the packers' output on the permuted w_okc, and the packers' own layouts are held by the existing packing tests.  What a wrong
row or K order would do to the bytes of a net is held end to end in tests/test_live_columns_gpu.py."""
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
    out = tmp_path_factory.mktemp("live_plan") / "call_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", str(SRC), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def _param():
    """[(w_okc [cout][25 cin], bias)] of the PARAM tables: k = tap cin + c, as the handle's d_w_okc holds them"""
    return [(w.reshape(w.shape[0], -1).astype(np.int8), b.astype(np.int8)) for w, b, _ in sicn_ref.load_param_fixture(GOLDEN)]


def _random(seed, n_dead):
    rng = np.random.default_rng(seed)
    net = []
    for cin, cout, *_ in NET:
        w = rng.integers(-8, 8, (cout, 25, cin)).astype(np.int8)
        if cin == 128 and n_dead:
            w[:, :, rng.permutation(128)[:n_dead]] = 0
        net.append((w.reshape(cout, -1), rng.integers(-128, 128, cout).astype(np.int8)))
    return net


def _run_rows(exe, d, weights, first=0, last=7, tap=3, meta=NET):
    """per layer the fields of its line as a dict, and the permutations of the layers that skip columns"""
    for l, (w, b) in enumerate(weights):
        w.tofile(d / f"l{l}.okc")
        b.tofile(d / f"l{l}.bias")
    (d / "meta.txt").write_text("".join(" ".join(map(str, m)) + "\n" for m in meta))
    r = subprocess.run([str(exe), str(d), str(len(weights)), str(first), str(last), str(tap)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr     # a sanitizer report ends the program with an error
    rows, perm = {}, {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "L":
            rows[int(f[1])] = {f[i]: int(f[i + 1]) for i in range(2, len(f), 2)}
        elif f[0] == "P":
            perm[int(f[1])] = [int(v) for v in f[2:]]
    return [rows[l] for l in range(len(weights))], perm


def _run(exe, d, weights, first=0, last=7, tap=3, meta=NET):
    rows, perm = _run_rows(exe, d, weights, first, last, tap, meta)
    return [r["live"] for r in rows], [r["nj"] for r in rows], perm


def _column(pos):
    return 4 * (pos >> 6) + ((pos >> 2) & 3)     # csrc/k_mfma16x.hip: column j = 4 J + d holds positions 64 J + 16 g + 4 d + r


def _check_images(d, weights, nj, perm):
    """p is a permutation whose live prefix is ordered and fills the computed columns; the permuted copies are the numpy statement"""
    for l, p in perm.items():
        p = np.array(p)
        assert sorted(p.tolist()) == list(range(128))
        w_next = weights[l + 1][0].reshape(weights[l + 1][0].shape[0], 25, 128)
        alive = np.flatnonzero(np.any(w_next != 0, axis=(0, 1)))
        dead = np.setdiff1d(np.arange(128), alive)
        assert len(alive) <= 16 * nj[l]
        assert all(_column(int(v)) < nj[l] for v in p[alive]), "a live channel outside the computed columns"
        assert np.all(np.diff(p[alive]) > 0)
        assert sorted(p[dead].tolist()) == sorted(set(range(128)) - set(p[alive].tolist()))
        computed = sorted(pos for pos in range(128) if _column(pos) < nj[l])
        assert p[alive].tolist() == computed[:len(alive)], "the live channels fill the computed positions in order"
        # the producer: row p[c] is row c, bias likewise;  the consumer: K index tap 128 + p[c] is tap 128 + c
        w, b = weights[l]
        w_out = np.empty_like(w)
        b_out = np.empty_like(b)
        w_out[p], b_out[p] = w, b
        assert np.array_equal(np.fromfile(d / f"l{l}.out.okc", np.int8).reshape(w.shape), w_out)
        assert np.array_equal(np.fromfile(d / f"l{l}.out.bias", np.int8), b_out)
        k_in = np.empty_like(w_next)
        k_in[:, :, p] = w_next
        assert np.array_equal(np.fromfile(d / f"l{l + 1}.in.okc", np.int8).reshape(w_next.shape), k_in)
        # what the pair computes is unchanged: the consumer's weights at the positions nobody computes are zero
        uncomputed = [pos for pos in range(128) if _column(pos) >= nj[l]]
        assert not np.any(k_in[:, :, uncomputed])


def test_param_tables_full_call(exe, tmp_path):
    weights = _param()
    live, nj, perm = _run(exe, tmp_path, weights)
    assert [live[l] for l in (0, 1, 2, 4, 5)] == [80] * 5 and live[6] == 48 and live[3] == 192 and live[7] == 3, live
    assert [nj[l] for l in (1, 2, 5, 6)] == [5, 5, 5, 3] and [nj[l] for l in (0, 3, 4, 7)] == [8] * 4, nj
    assert sorted(perm) == [1, 2, 5, 6]
    _check_images(tmp_path, weights, nj, perm)
    # the dead channels are the residue classes the tables have
    dead = lambda l: set(np.flatnonzero(~np.any(weights[l][0].reshape(-1, 25, weights[l][0].shape[1] // 25) != 0, axis=(0, 1))).tolist())
    assert dead(2) == {c for c in range(128) if c % 8 >= 5} and dead(7) == {c for c in range(128) if c % 8 >= 3}
    assert dead(4) == {c for c in range(192) if c % 12 >= 5}


def test_tapped_and_last_layers_keep_every_column(exe, tmp_path):
    live, nj, perm = _run(exe, tmp_path, _param(), 0, 7, 1)
    assert nj[1] == 8 and live[1] == 128 and 1 not in perm and nj[2] == 5, (live, nj)     # layers 1 and 2 use the standard images
    live, nj, perm = _run(exe, tmp_path, _param(), 4, 6, -1)
    assert nj == [8, 8, 8, 8, 8, 5, 8, 8] and sorted(perm) == [5], nj


def test_gdn_and_other_families_keep_every_column(exe, tmp_path):
    meta = [list(m) for m in NET]
    meta[1][2] = 1        # a GDN on layer 1
    meta[5][3] = 0        # layer 5 not planned onto the wide family in this call
    live, nj, perm = _run(exe, tmp_path, _param(), meta=meta)
    assert nj[1] == 8 and live[1] == 128 and nj[5] == 8 and nj[2] == 5 and nj[6] == 3 and sorted(perm) == [2, 6], (live, nj)


def test_halves_and_walk_of_the_param_tables(exe, tmp_path):
    """layer 7 behind at most 4 columns in the GROUP or PHASE layout reads 1 half, otherwise 2; a wide conv behind three groups walks 3
    groups, a deconv 4"""
    rows, _ = _run_rows(exe, tmp_path, _param())
    assert rows[6]["nj"] == 3 and [r["halves"] for r in rows] == [2] * 7 + [1], rows
    assert rows[0]["groups"] == 3 and [r["walk"] for r in rows] == [4, 3] + [4] * 6, rows
    for layout, halves in ((1, 1), (0, 2)):
        meta = [list(m) for m in NET]
        meta[6][4] = layout       # layer 6 hands layer 7 the GROUP layout / NHWC
        rows, _ = _run_rows(exe, tmp_path, _param(), meta=meta)
        assert rows[6]["nj"] == 3 and rows[7]["halves"] == halves, rows[7]
    rows, _ = _run_rows(exe, tmp_path, _param(), 4, 7, -1)      # layer 5 runs 5 columns, layer 6 3: only layer 7 reads a half
    assert [r["halves"] for r in rows] == [2] * 7 + [1] and [r["walk"] for r in rows] == [4] * 8, rows
    rows, _ = _run_rows(exe, tmp_path, _param(), 0, 7, 6)       # a tap at layer 6: it computes all 8 columns and leaves in NHWC
    assert rows[6]["nj"] == 8 and rows[7]["halves"] == 2, rows
    meta = [list(m) for m in NET]
    meta[1][5] = 1                # layer 1 as a deconv behind layer 0's three groups
    rows, _ = _run_rows(exe, tmp_path, _param(), meta=meta)
    assert (rows[0]["groups"], rows[1]["groups_in"], rows[1]["walk"]) == (3, 3, 4), rows[1]
    meta = [list(m) for m in NET]
    meta[1][3] = 0                # layer 1 not on the wide family
    rows, _ = _run_rows(exe, tmp_path, _param(), meta=meta)
    assert (rows[1]["groups_in"], rows[1]["walk"]) == (3, 4), rows[1]


@pytest.mark.parametrize("n_dead, want", [(0, 8), (47, 8), (48, 5), (79, 5), (80, 3), (112, 3), (127, 3)])
def test_random_weights(exe, tmp_path, n_dead, want):
    """dense weights skip nothing; 81 live channels are 6 columns, which run on the next width that is built: all 8"""
    weights = _random(n_dead, n_dead)
    rows, perm = _run_rows(exe, tmp_path, weights)
    live, nj = [r["live"] for r in rows], [r["nj"] for r in rows]
    assert rows[7]["halves"] == (1 if want == 3 else 2) and [r["halves"] for r in rows[:7]] == [2] * 7, rows
    assert rows[1]["walk"] == (3 if 128 - n_dead <= 96 else 4) and [r["walk"] for r in rows[2:]] == [4] * 6, rows
    assert [nj[l] for l in (1, 2, 5, 6)] == [want] * 4 and [nj[l] for l in (0, 3, 4, 7)] == [8] * 4, nj
    assert [live[l] for l in (0, 1, 2, 5, 6)] == [128 - n_dead] * 5
    assert sorted(perm) == ([1, 2, 5, 6] if want < 8 else [])
    _check_images(tmp_path, weights, nj, perm)


def test_kernel_names_are_what_they_were():
    """sicn_kernel_for answers as before the plan existed: skipping columns is a matter of a net's call, not of a layer's family
    (needs the built library, no GPU; that dense weights keep all 8 columns is test_random_weights[0-8] and the GPU file's `dense`)"""
    import ctypes
    from simple_image_compression_network_amd import _lib
    from simple_image_compression_network_amd.config import eight_layer_descs
    names = [_lib.lib().sicn_kernel_for(ctypes.byref(d.to_c())).decode() for d in eight_layer_descs(768, 512)]
    assert names == ["l0_rgb", "mfma_conv", "mfma_conv", "mfma_conv", "mfma_deconv", "mfma_deconv", "mfma_deconv", "l7_rgb"]
