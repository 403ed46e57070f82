"""GPU cases that only make sense in a process whose library plans for a FORCED chip size (SICN_N_CU, read once at load) or with
the dynamic tile deal switched off (SICN_NO_DEAL=1).  tests/test_partition_plans.py starts one child pytest per CU count and hands
it this file by path, in front of the existing tests it re-runs; in an ordinary session, where neither variable is set, every
test here skips.  Byte equality throughout: the path is integer."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import LayerDesc

ROOT = Path(__file__).resolve().parent.parent
FORCED_CU = int(os.environ.get("SICN_N_CU") or 0)
NO_DEAL = (os.environ.get("SICN_NO_DEAL") or "0") != "0"
N_XCD = {32: 1, 64: 2, 128: 4, 240: 8, 256: 8}      # include/sicn.h: the largest power of two <= 8 with >= 20 CUs per XCD

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not FORCED_CU and not NO_DEAL, reason="runs in the child sessions of test_partition_plans.py only "
                                                                        "(SICN_N_CU / SICN_NO_DEAL are read when the library loads)")]

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import api as _api
    return _api


def _chip(api):
    out = (ctypes.c_int32 * 2)()
    assert api._lib.lib().sicn_debug_chip(out) == 0
    return int(out[0]), int(out[1])


def _plan(api, d, n_images, n_cu, **opts):
    out = (ctypes.c_int32 * 12)()
    o = api._lib.make_options(**opts)
    assert api._lib.lib().sicn_debug_plan(ctypes.byref(d.to_c()), n_images, ctypes.byref(o), n_cu, out) == 0
    keys = ("n_cu", "n_xcd", "kind", "family", "tile_x", "split_n", "split_k", "gx", "gy", "gz", "chunks", "ty_per")
    return dict(zip(keys, list(out)))


def test_the_library_plans_with_the_forced_chip(api):
    """First test of every child session: without it the whole session could pass while planning for the real chip.  It launches
    nothing."""
    device_cus = torch.cuda.get_device_properties(0).multi_processor_count
    want_cu = FORCED_CU or device_cus
    assert want_cu in N_XCD, f"no XCD count on record for {want_cu} CUs"
    assert _chip(api) == (want_cu, N_XCD[want_cu])
    if FORCED_CU:
        assert FORCED_CU != device_cus, "forcing the device's own CU count tests nothing"
    print(f"partition child: n_cu={want_cu} n_xcd={N_XCD[want_cu]} no_deal={int(NO_DEAL)}")


@pytest.mark.parametrize("transposed", [0, 1], ids=["conv", "deconv"])
def test_automatic_wide_deal_on_the_forced_chip(api, transposed):
    """conv / deconv 128 -> 128 as a one-layer net at the DEFAULT grid, with 16 tiles of 16 x 32 positions per workgroup: the planner
    itself picks the wide persistent kernel, one workgroup per CU of the forced chip, and the dynamic deal (k_mfma16x.hip DealX) with
    one ticket counter per XCD of the forced chip — 1 / 2 / 4 counters on 32 / 64 / 128 workgroups.  From 240 CUs on the oracle
    would have to compute 3840 tiles; there (and in the SICN_NO_DEAL session, which plans for the whole chip) the grid is capped at
    64 workgroups, so the planned deal still has 8 counters.  Three calls and two graph replays against the C oracle's direct form:
    a lost or doubled tile shows in the bytes."""
    n_cu, n_xcd = _chip(api)
    opts = {} if n_cu <= 128 else {"wave_tile": 128, "persistent_grid": 64}
    groups = n_cu if n_cu <= 128 else 64
    n = 2
    tx, ty = 16, groups // 2                                 # tx * ty * n = 16 * groups tiles, the last column and row ragged
    mw, mh = 32 * tx - 5, 16 * ty - 3
    w, h = (mw, mh) if transposed else (2 * mw - 1, 2 * mh)
    d = LayerDesc.make(128, 128, 8, 16, w, h, transposed)
    p = _plan(api, d, n, n_cu, **opts)
    assert (p["kind"], p["family"], p["gx"], p["chunks"], p["n_xcd"]) == (2 if transposed else 1, 2, groups, 1, n_xcd), p
    rng = np.random.default_rng([41, n_cu, transposed])
    W = rng.integers(-8, 8, (128, 5, 5, 128)).astype(np.int8)
    b = rng.integers(-128, 128, 128).astype(np.int8)
    words = sicn_ref.pack_finn_tiles(W, 8, 16)
    x = rng.integers(0, 128, (n,) + d.in_shape, dtype=np.uint8)
    x[1].reshape(-1)[::7] |= 0x80
    ref = np.stack([c_oracle.run_layer(d, words, b, x[i], "direct", threads=min(16, os.cpu_count() or 1)) for i in range(n)])
    assert np.count_nonzero(ref) > ref.size // 8
    fpw = api.FixedPointWeights(8, 4, 16, d.W_TILES, words)
    net = api.EightLayersNet(descs=[d], params=[(fpw, b)], options=opts or None)
    xin = torch.from_numpy(x).cuda()
    out = None
    for call in range(3):
        out, _ = net.run_layers(0, 0, xin)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got, ref), f"call {call}: {np.count_nonzero(got != ref)} of {ref.size} bytes differ"
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            net.run_layers(0, 0, xin, out=out)
    for replay in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got, ref), f"replay {replay}: {np.count_nonzero(got != ref)} of {ref.size} bytes differ"


def test_randomised_sweep_on_the_forced_chip(api):
    """tests/fuzz_parity.py with a seed of this chip size, in a child process that inherits the forced count: layers, chains
    (mixed kernel families among them), the fused layer-0 activation and the dynamic deal, whose grid the script sizes from
    sicn_debug_chip."""
    n_cu, _ = _chip(api)
    seed = 1000 + n_cu + (7 if NO_DEAL else 0)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "fuzz_parity.py"), "--cases", "60", "--chains", "4", "--gdn", "10",
                        "--deal", "4", "--seed", str(seed)], capture_output=True, text=True, timeout=900, cwd=str(ROOT))
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    for line in ("60/60 cases bit-exact", "4/4 chains bit-exact", "10/10 fused-activation cases bit-exact", "4/4 dynamic-deal cases bit-exact"):
        assert line in r.stdout, line
