"""The launch plans of a partitioned chip, RUN on the GPU.

include/sicn.h ("Device") and csrc/sicn_plan.h promise that every grid, strip cut, tile width, channel split, the wide / pipelined
choice and the XCD-aware work list follow the device's CU count (DPX 128 CUs / 4 XCDs, QPX 64 / 2, CPX 32 / 1, a part with
fused-off CUs such as 240 / 8); n_xcd is a kernel argument.  tests/test_abi_load.py walks those plans as numbers; an ordinary
GPU session only ever launches the plans of the whole chip.  SICN_N_CU=n (read once, when the library loads) makes the library
plan for n CUs on whatever chip it runs on, so this module starts one child pytest per CU count — and one with SICN_NO_DEAL=1 —
over tests/test_partition_cases.py and a list of existing tests whose path depends on the plan.

The CPU half keeps the GPU half from becoming vacuous: a committed table of plan fields that must differ between the forced
count and 256 CUs for the sizes the re-run tests use, the option defaults read from the environment, and the existence of every
listed node id."""
import ctypes
import os
import signal
import subprocess
import sys
from pathlib import Path

import pytest

from simple_image_compression_network_amd import _lib
from simple_image_compression_network_amd.config import LayerDesc, eight_layer_descs

ROOT = Path(__file__).resolve().parent.parent

PARTITIONS = (32, 64, 128, 240)
N_XCD = {32: 1, 64: 2, 128: 4, 240: 8}

_KEYS = ("n_cu", "n_xcd", "kind", "family", "tile_x", "split_n", "split_k", "gx", "gy", "gz", "chunks", "ty_per")


def _plan(d, n_images, n_cu, **opts):
    out = (ctypes.c_int32 * 12)()
    o = _lib.make_options(**opts)
    assert _lib.lib().sicn_debug_plan(ctypes.byref(d.to_c()), n_images, ctypes.byref(o), n_cu, out) == 0
    return dict(zip(_KEYS, list(out)))


# (n_cu, (width, height), batch, layer, plan field): the field differs from its value on 256 CUs.  The sizes are those of the
# tests the children re-run (1080p closed form, the 768 x 512 chains and hashes, the 256 x 256 hashes).  For layer 0 "gy" is the
# number of runs per strip, for layer 7 "chunks" the cuts per strip, for the MFMA layers "family" 1 = pipelined, 2 = wide persistent.
PLAN_DIFFERS = [
    (32, (1920, 1080), 1, 0, "gy"), (32, (1920, 1080), 1, 1, "family"), (32, (1920, 1080), 1, 6, "family"),
    (32, (1920, 1080), 1, 1, "gx"), (32, (1920, 1080), 1, 2, "tile_x"), (32, (1920, 1080), 1, 5, "tile_x"),
    (32, (1920, 1080), 1, 3, "split_n"), (32, (1920, 1080), 1, 4, "split_n"), (32, (1920, 1080), 1, 7, "chunks"),
    (64, (1920, 1080), 1, 0, "gy"), (64, (1920, 1080), 1, 1, "family"), (64, (1920, 1080), 1, 7, "chunks"),
    (128, (1920, 1080), 1, 0, "gy"), (128, (1920, 1080), 1, 3, "split_n"), (128, (1920, 1080), 1, 4, "split_n"),
    (128, (1920, 1080), 1, 7, "chunks"),
    (240, (1920, 1080), 1, 0, "gy"), (240, (1920, 1080), 1, 7, "chunks"),
    (32, (768, 512), 2, 0, "gy"), (32, (768, 512), 2, 1, "tile_x"), (32, (768, 512), 2, 6, "tile_x"),
    (32, (768, 512), 2, 2, "split_n"), (32, (768, 512), 2, 3, "split_n"), (32, (768, 512), 2, 4, "split_n"),
    (32, (768, 512), 2, 5, "split_n"), (32, (768, 512), 2, 7, "chunks"),
    (64, (768, 512), 2, 0, "gy"), (64, (768, 512), 2, 1, "tile_x"), (64, (768, 512), 2, 6, "tile_x"),
    (64, (768, 512), 2, 2, "split_n"), (64, (768, 512), 2, 5, "split_n"), (64, (768, 512), 2, 7, "chunks"),
    (128, (768, 512), 2, 0, "gy"), (128, (768, 512), 2, 2, "split_n"), (128, (768, 512), 2, 5, "split_n"),
    (128, (768, 512), 2, 7, "chunks"),
    (240, (768, 512), 2, 7, "chunks"),
    (32, (256, 256), 1, 1, "split_n"), (32, (256, 256), 1, 6, "split_n"), (32, (256, 256), 1, 3, "gx"), (32, (256, 256), 1, 4, "gx"),
    (32, (256, 256), 1, 7, "chunks"),
    (64, (256, 256), 1, 3, "gx"), (64, (256, 256), 1, 4, "gx"),
    (128, (256, 256), 1, 3, "gx"), (128, (256, 256), 1, 4, "gx"),
]


def test_partition_xcd_counts():
    d = eight_layer_descs(256, 256)[0]
    assert tuple(_plan(d, 1, n)["n_xcd"] for n in PARTITIONS) == (1, 2, 4, 8)
    assert all(_plan(d, 1, n)["n_xcd"] == N_XCD[n] and _plan(d, 1, n)["n_cu"] == n for n in PARTITIONS)
    assert _plan(d, 1, 256)["n_xcd"] == 8


@pytest.mark.parametrize("n_cu", PARTITIONS)
def test_forced_plans_differ_from_the_whole_chip(n_cu):
    """If planning changes so that a partition launches what the whole chip launches, the children below test nothing new: every
    entry must still differ, and every partition but the 240-CU part must differ at every size."""
    entries = [e for e in PLAN_DIFFERS if e[0] == n_cu]
    assert {e[1] for e in entries} >= ({(1920, 1080), (768, 512)} | (set() if n_cu == 240 else {(256, 256)}))
    for _, size, batch, layer, field in entries:
        d = eight_layer_descs(*size)[layer]
        forced, whole = _plan(d, batch, n_cu), _plan(d, batch, 256)
        assert forced[field] != whole[field], (n_cu, size, batch, layer, field, forced, whole)


def test_forced_plans_match_the_recorded_numbers():
    """A few of the numbers behind the table, so that the table is known to say what it was written for."""
    d1080, d768 = eight_layer_descs(1920, 1080), eight_layer_descs(768, 512)
    assert [_plan(d1080[0], 1, n)["gy"] for n in (256, 240, 128, 64, 32)] == [34, 23, 17, 9, 8]
    assert _plan(d1080[0], 1, 32)["ty_per"] == 9
    assert [_plan(d1080[7], 1, n)["chunks"] for n in (256, 240, 128, 64, 32)] == [17, 16, 8, 4, 2]
    assert [_plan(d768[7], 2, n)["chunks"] for n in (256, 240, 128, 64, 32)] == [21, 20, 10, 5, 2]
    assert [_plan(d768[0], 2, n)["gy"] for n in (256, 128, 64, 32)] == [32, 16, 11, 6]
    p = _plan(d1080[1], 1, 32)
    assert (p["family"], p["gx"], p["n_xcd"]) == (2, 32, 1)
    p = _plan(d1080[1], 1, 64)
    assert (p["family"], p["gx"], p["n_xcd"]) == (2, 64, 2)
    assert _plan(d1080[6], 1, 64)["family"] == 1 and _plan(d1080[6], 1, 32)["family"] == 2
    assert _plan(d1080[1], 1, 256)["family"] == 1 and _plan(d1080[6], 1, 256)["family"] == 1
    # the forced wide grid of test_wide_kernels_dynamic_tile_deal_matches_oracle: 8 workgroups on 1 / 2 / 4 / 8 ticket counters
    d = LayerDesc.make(128, 128, 8, 16, 512, 200, 0)
    for n_cu, n_xcd in ((32, 1), (64, 2), (128, 4), (240, 8), (256, 8)):
        p = _plan(d, 3, n_cu, wave_tile=128, persistent_grid=8)
        assert (p["family"], p["gx"], p["n_xcd"], p["chunks"]) == (2, 8, n_xcd, 1), (n_cu, p)


def test_option_defaults_come_from_the_environment_at_load():
    """default_options() reads SICN_<FIELD> once, when the library loads: a child process with the variables set sees them in
    sicn_options_init, force_generic is normalised to 0 / 1, and a value the field does not admit is ignored with one line on
    stderr."""
    code = ("import ctypes\n"
            "from simple_image_compression_network_amd import _lib\n"
            "o = _lib.COptions()\n"
            "_lib.lib().sicn_options_init(ctypes.byref(o))\n"
            "print('OPTS', o.tile_x, o.prefetch, o.wave_tile, o.strip_chunks, o.force_generic, o.split_n)\n")
    env = dict(os.environ, SICN_TILE_X="16", SICN_PREFETCH="2", SICN_WAVE_TILE="64", SICN_STRIP_CHUNKS="3", SICN_FORCE_GENERIC="5",
               SICN_SPLIT_N="9")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OPTS 16 2 64 3 1 0" in r.stdout.splitlines(), r.stdout
    assert "libsicn: ignoring out-of-range SICN_SPLIT_N=9" in r.stderr.splitlines(), r.stderr


def test_debug_chip_needs_a_device_or_says_so():
    """sicn_debug_chip: {n_cu, n_xcd} of the current device as the library plans with it, SICN_ENODEV without one; a null pointer is
    refused before any device is asked."""
    L = _lib.lib()
    assert L.sicn_debug_chip(None) == -22
    out = (ctypes.c_int32 * 2)()
    rc = L.sicn_debug_chip(out)
    assert rc in (0, -19)
    if rc == 0:
        assert out[0] >= 1 and out[1] in (1, 2, 4, 8)
    else:
        assert list(out) == [0, 0]


# ---- the children -------------------------------------------------------------------------------------------------------------
# tests/test_partition_cases.py first: its first test asserts the forced chip.  Then existing tests with small inputs whose path
# depends on the plan (a function id selects every parametrisation).  Left out: the 4K tests, the bench.py subprocess tests, the
# C++ testbench.  Thinned once, because the five children more than doubled the GPU suite: of the two largest parametrised tests
# only prefetch = 2 runs (prefetch = 1 plans exactly what 2 does, test_abi_load.py asserts it), and tests that no plan reaches
# differently (the workspace of the old size, which forces its own grid) are not re-run.
_PARITY = "tests/test_gpu_parity.py::"
CHILD_IDS = ["tests/test_partition_cases.py"] + [_PARITY + t for t in (
    "test_layer_matches_oracle_random_weights", "test_strip_kernels_long_strips",
    "test_output_channel_split_matches_oracle", "test_output_channel_split_in_chain",
    "test_wide_kernels_dynamic_tile_deal_matches_oracle",
    "test_persistent_conv_matches_oracle", "test_persistent_conv_in_chain", "test_wide_wave_tile_conv_matches_oracle",
    "test_wide_wave_tile_deconv_matches_oracle", "test_wide_wave_tile_in_chain",
    "test_pipelined_kernels_in_chain", "test_both_tile_widths_in_chain", "test_eight_layers_net_matches_reference_hashes",
    "test_1080p_full_net_matches_closed_form", "test_forward_is_graph_capturable", "test_capture_helper_replays",
    "test_persistent_kernels_graph_replay_and_two_streams")] + [
    f"{_PARITY}test_both_tile_widths_match_oracle[case{c}-{tile_x}-2]" for c in range(18) for tile_x in (16, 32)] + [
    f"{_PARITY}test_pipelined_kernels_match_oracle[case{c}-2]" for c in range(13)] + [f"tests/test_gdn.py::{t}" for t in (
        "test_gpu_layer_with_gdn_equals_oracle", "test_gpu_gdn_net_all_internal_layouts",
        "test_gpu_layer0_with_gdn_in_one_kernel_equals_oracle", "test_gpu_layer0_with_gdn_in_one_kernel_at_1080p")] + [
    f"tests/test_codec.py::{t}" for t in (
        "test_gpu_container_equals_oracle_and_round_trips", "test_gpu_batch_equals_single_calls_and_oracle",
        "test_gpu_async_pair_equals_sync_and_oracle", "test_gpu_async_decode_with_many_streams_takes_the_scan_path")] + [
    "tests/test_hyperprior.py::test_gpu_hyperprior_pipeline_equals_oracle_stage_by_stage",
    "tests/test_any_width_gpu.py::test_whole_net_at_other_widths",
]


def test_every_listed_node_id_exists():
    """A renamed test must not drop out of the children silently: one collection over the list, every id must collect something."""
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + CHILD_IDS,
                       capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    collected = [ln.strip() for ln in r.stdout.splitlines() if "::" in ln]
    assert len(CHILD_IDS) == len(set(CHILD_IDS))
    for node in CHILD_IDS:
        assert any(c == node or c.startswith(node + "[") or c.startswith(node + "::") for c in collected), f"{node} collects nothing"


# Time limit of one child.  Measured on an MI355X with the parent commit's kernels: the selection, no variable set, took 39 s of
# wall time before it was thinned (CHILD_UNFORCED_S) and 35 s after; every child gets three times that, rounded up to whole
# minutes = 120 s either way (the forced plans put as little as an eighth of the workgroups on a layer, but most of the time is
# the oracle on the CPU).  The children themselves took 44 - 53 s (49 - 59 s before the thinning): the test_partition_cases.py
# part, which skips without a variable, is the difference.
CHILD_UNFORCED_S = 39
CHILD_TIMEOUT_S = -(-3 * CHILD_UNFORCED_S // 60) * 60

# exit statuses after which nothing more is started on the GPU: a signal or abort, or a time limit
_FATAL = (-6, -11, 124, 134, 137, 139)
_latch = {"why": None}


def _run_child(env_extra):
    if _latch["why"]:
        pytest.fail("not started: an earlier child session ended abnormally\n" + _latch["why"], pytrace=False)
    env = dict(os.environ, **env_extra)
    for name in ("SICN_N_CU", "SICN_NO_DEAL"):
        if name not in env_extra:
            env.pop(name, None)
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider"] + CHILD_IDS
    # a session of its own, so that a time limit ends the child together with whatever it started (the fuzz script)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=str(ROOT), start_new_session=True)
    try:
        stdout, stderr = proc.communicate(timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        stdout, stderr = proc.communicate()
        _latch["why"] = f"child {env_extra} ran into its time limit of {CHILD_TIMEOUT_S} s\n{(stdout or '')[-3000:]}"
        pytest.fail(_latch["why"], pytrace=False)
    tail = stdout[-4000:] + "\n" + stderr[-2000:]
    if proc.returncode < 0 or proc.returncode in _FATAL:
        _latch["why"] = f"child {env_extra} ended with status {proc.returncode}\n{tail}"
        pytest.fail(_latch["why"], pytrace=False)
    assert proc.returncode == 0, f"child {env_extra} failed (status {proc.returncode})\n{tail}"
    return stdout


def _assert_child_report(out, n_cu, n_xcd, no_deal):
    assert f"partition child: n_cu={n_cu} n_xcd={n_xcd} no_deal={no_deal}" in out, out[-2000:]
    for line in ("60/60 cases bit-exact", "4/4 chains bit-exact", "10/10 fused-activation cases bit-exact", "4/4 dynamic-deal cases bit-exact"):
        assert line in out, (line, out[-2000:])
    assert " skipped" not in out.splitlines()[-1], out.splitlines()[-1]      # with a variable set nothing in the selection skips


@pytest.mark.gpu
@pytest.mark.parametrize("n_cu", PARTITIONS)
def test_gpu_partition_plans_run(n_cu):
    """One child session whose library plans for n_cu CUs: it asserts that first (sicn_debug_chip), then runs the selection."""
    out = _run_child({"SICN_N_CU": str(n_cu)})
    _assert_child_report(out, n_cu, N_XCD[n_cu], 0)


@pytest.mark.gpu
def test_gpu_static_deal_switch_runs():
    """SICN_NO_DEAL=1: the wide persistent kernels deal every tile statically even inside a net with a workspace."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    out = _run_child({"SICN_NO_DEAL": "1"})
    _assert_child_report(out, n_cu, _plan(eight_layer_descs(256, 256)[0], 1, n_cu)["n_xcd"], 1)
