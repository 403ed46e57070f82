#!/usr/bin/env python3
"""Randomised parity sweep: every kernel family on random image sizes / batch sizes / strip cuts / tile widths against
the numpy closed form (oracle/sicn_ref.py), bit for bit; where that form's float32 sums would not be exact (many channels, input
bytes above 127) against the C oracle's direct form, which is integer.  usage: fuzz_parity.py [--cases N] [--seed S]"""
import argparse
import ctypes
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import c_oracle, sicn_ref  # noqa: E402  (checkers)
from simple_image_compression_network_amd import _lib, api  # noqa: E402
from simple_image_compression_network_amd.config import LayerDesc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=200)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--big", action="store_true", help="image sizes up to 600 x 400 (slow on the CPU side)")
ap.add_argument("--chains", type=int, default=0, help="additionally: whole 8-layer chains (internal layouts) on random sizes")
ap.add_argument("--gdn", type=int, default=0, help="additionally: layer 0 + GDN in one kernel (k_l0g), random sizes, against the C oracle of the GDN")
ap.add_argument("--deal", type=int, default=0, help="additionally: one-layer nets of conv / deconv 128 -> 128 on few wide persistent workgroups that walk >= 16 "
                "tiles each, so that the dynamic part of the tile deal (k_mfma16x.hip DealX: tickets, stealing across XCDs) is what runs; three "
                "calls + a graph replay each")
ap.add_argument("--live", type=int, default=0, help="additionally: two-layer nets, conv / deconv 128 -> 128 in front of a consumer with 112 .. 0 dead input channels, so "
                "that the producer runs the live-column kernels (k_mfma16x_live.hip: 3 / 5 / 8 accumulator columns) and a deconv 128 -> 3 behind 3 "
                "columns reads one channel half; 1 .. 6 x 1 .. 6 ragged tiles, 8 / 16 / all workgroups, against the C oracle")
args = ap.parse_args()
rng = np.random.default_rng(args.seed)

THREADS = min(16, os.cpu_count() or 1)


def layer_ref(d, W, b, words, x):
    """One image through one layer: the numpy closed form while its float32 GEMM is exact (sicn_ref._exact_gemm_ok), else the C oracle."""
    if 25 * d.IFM_CH * (int(x.max()) if x.size else 0) * 8 < (1 << 24):
        return (sicn_ref.deconv522_ref if d.transposed else sicn_ref.conv2d_ref)(x, W, b)
    return c_oracle.run_layer(d, words, b, x, form="direct", threads=THREADS)


def kernel_for(d):
    return _lib.lib().sicn_kernel_for(ctypes.byref(d.to_c())).decode()


FAMILIES = [  # (cin, cout, simd, pe, transposed)
    (3, 128, 3, 8, 0), (128, 128, 8, 16, 0), (128, 192, 8, 24, 0), (192, 128, 12, 16, 1), (128, 128, 8, 16, 1), (128, 3, 8, 3, 1)]
bad = 0
for case in range(args.cases):
    any_width = rng.random() < 0.3          # the channel-generic kernels (k_mfma16c.hip): IFM_CH a multiple of 32, OFM_CH of 16, up to 1024
    if any_width:
        tr = int(rng.integers(2))
        cin, cout = 32 * int(rng.integers(1, 33)), 16 * int(rng.integers(1, 65))
        end = rng.random()
        if end < 0.15:                      # the RGB ends at other widths
            (cin, cout) = (cin, 3) if tr else (3, cout)
        simd, pe = (3 if cin == 3 else 8), (3 if cout == 3 else 16)
    else:
        cin, cout, simd, pe, tr = FAMILIES[rng.integers(len(FAMILIES))]
    big = rng.random() < 0.25 and not (any_width and cin * cout > 256 * 256)      # the CPU side of a wide layer is slow
    w = int(rng.integers(1, 600 if args.big else 200 if big else 70))
    h = int(rng.integers(1, 400 if args.big else 120 if big else 40))
    if cin == 3:
        w, h = w * 2 + int(rng.integers(2)), h * 2 + int(rng.integers(2))
    n = int(rng.integers(1, 4))
    d = LayerDesc.make(cin, cout, simd, pe, w, h, tr)
    if any_width and kernel_for(d) in ("generic", "invalid", "mfma_conv", "mfma_deconv", "l0_rgb", "l7_rgb"):
        any_width = False        # a draw that hit one of the specialised shapes: it runs, as one of theirs
    env = {}                     # sicn_options fields, per call
    if rng.random() < 0.5:
        env["strip_chunks"] = int(rng.integers(1, 9))
    if rng.random() < 0.5:
        env["tile_x"] = int(rng.choice([16, 32]))
    if rng.random() < 0.3:
        env["split_n"] = int(rng.choice([1, 2, 4]))
    if cin != 3 and rng.random() < 0.4:       # the wide persistent kernels (only conv / deconv 128 -> 128 take them; others ignore the request)
        env["wave_tile"] = 128
        env["tile_x"] = 32
        env["persistent_grid"] = int(rng.choice([8, 16, 64, 0]))
    W = rng.integers(-8, 8, (cout, 5, 5, cin)).astype(np.int8)
    b = rng.integers(-128, 128, cout).astype(np.int8)
    words = sicn_ref.pack_finn_tiles(W, simd, pe)
    x = rng.integers(0, 256 if cin == 3 or (any_width and rng.random() < 0.5) else 128, (n,) + d.in_shape, dtype=np.uint8)
    if cin != 3 and rng.random() < 0.3:
        x.reshape(-1)[::5] |= 0x80
    fpw = api.FixedPointWeights(simd, 4, pe, d.W_TILES, words)
    fn = api.deconv522 if tr else api.conv2d
    got = fn(d, fpw, b, torch.from_numpy(x).cuda(), None, n, options=env or None)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    ok = all(np.array_equal(got[i], layer_ref(d, W, b, words, x[i])) for i in range(n))
    if not ok:
        bad += 1
        print(f"MISMATCH case {case}: cin={cin} cout={cout} tr={tr} w={w} h={h} n={n} env={env}", flush=True)
    elif case % 25 == 0:
        print(f"case {case}: ok (cin={cin} cout={cout} tr={tr} {w}x{h} n={n} {env})", flush=True)
print(f"{args.cases - bad}/{args.cases} cases bit-exact")

# whole chains: random image sizes, random nibble weights, latent + reconstruction against the closed form
from simple_image_compression_network_amd.config import eight_layer_descs  # noqa: E402
CHAIN_WIDTHS = [(128, 192), (128, 256), (192, 128), (64, 96), (128, 64)]
cbad = 0
for case in range(args.chains):
    env = {}
    if rng.random() < 0.5:
        env["tile_x"] = int(rng.choice([16, 32]))
    if rng.random() < 0.5:
        env["strip_chunks"] = int(rng.integers(1, 6))
    if rng.random() < 0.3:
        env["split_n"] = int(rng.choice([1, 2, 4]))
    if rng.random() < 0.4:
        env["wave_tile"] = 128
        env["tile_x"] = 32
        env["persistent_grid"] = int(rng.choice([8, 16, 64, 0]))
    w, h, n = int(rng.integers(1, 26)) * 16, int(rng.integers(1, 20)) * 16, int(rng.integers(1, 3))
    # the reference widths, nets that mix the specialised kernel families with the channel-generic ones, and one all channel-generic
    n_ch, m_ch = CHAIN_WIDTHS[rng.integers(len(CHAIN_WIDTHS))]
    descs = eight_layer_descs(w, h, n_ch, m_ch)
    params_np, params = [], []
    for d in descs:
        Wt = rng.integers(-8, 8, (d.OFM_CH, 5, 5, d.IFM_CH)).astype(np.int8)
        bt = rng.integers(-128, 128, d.OFM_CH).astype(np.int8)
        params_np.append((Wt, bt, sicn_ref.pack_finn_tiles(Wt, d.SIMD, d.PE)))
        params.append((api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, params_np[-1][2]),
                       api.FixedPointWeights(1, 8, 1, d.OFM_CH, bt.view(np.uint8).astype(np.uint64))))
    net = api.EightLayersNet(descs=descs, params=params, options=env or None)
    x = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    out, lat = net.forward(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    out, lat = out.cpu().numpy(), lat.cpu().numpy()
    ok = True
    for i in range(n):
        ref = [x[i]]
        for d, (Wt, bt, words) in zip(descs, params_np):
            ref.append(layer_ref(d, Wt, bt, words, ref[-1]))
        ok = ok and np.array_equal(out[i], ref[8]) and np.array_equal(lat[i], ref[4])
    if not ok:
        cbad += 1
        print(f"CHAIN MISMATCH {case}: {w}x{h} n={n} widths=({n_ch}, {m_ch}) env={env}", flush=True)
    elif case % 5 == 0:
        print(f"chain {case}: ok ({w}x{h} n={n} widths=({n_ch}, {m_ch}))", flush=True)
if args.chains:
    print(f"{args.chains - cbad}/{args.chains} chains bit-exact")

# the activation inside the layer kernels (extension beyond the reference): against oracle/sicn_gdn_oracle.c
gbad = 0
for case in range(args.gdn):
    inverse = bool(rng.integers(2))
    beta = rng.integers(1, 65536, 128).astype(np.uint32)
    gamma = rng.integers(0, 128, (128, 128)).astype(np.uint8)
    if rng.random() < 0.5:
        gamma = (gamma >> 4).astype(np.uint8)
    env = {}
    if rng.random() < 0.5:
        env["strip_chunks"] = int(rng.integers(1, 7))
    n = int(rng.integers(1, 4))
    def mk(cin, cout, simd, pe, w, h, tr):
        d = LayerDesc.make(cin, cout, simd, pe, w, h, tr)
        Wt = rng.integers(-8, 8, (cout, 5, 5, cin)).astype(np.int8)
        bt = rng.integers(-128, 128, cout).astype(np.int8)
        return d, Wt, bt
    d, Wt, bt = mk(3, 128, 3, 8, int(rng.integers(1, 300)), int(rng.integers(1, 200)), 0)
    x = rng.integers(0, 256, (n,) + d.in_shape, dtype=np.uint8)
    g = api.GDN(beta, gamma, inverse, 12)
    fpw = api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, sicn_ref.pack_finn_tiles(Wt, d.SIMD, d.PE))
    got = api.conv2d(d, fpw, bt, torch.from_numpy(x).cuda(), None, n, gdn=g, options=env or None).cpu().numpy()
    ok = all(np.array_equal(got[i], c_oracle.gdn(sicn_ref.layer_preact_ref(x[i], Wt, bt, 0), beta, gamma, inverse, 12)) for i in range(n))
    what = f"k_l0g {d.IFM_ROW}x{d.IFM_COL}"
    if not ok:
        gbad += 1
        print(f"GDN MISMATCH {case}: {what} n={n} inverse={inverse} env={env}", flush=True)
    elif case % 10 == 0:
        print(f"gdn {case}: ok ({what} n={n} inverse={inverse} {env})", flush=True)
if args.gdn:
    print(f"{args.gdn - gbad}/{args.gdn} fused-activation cases bit-exact")
# the wide kernels' dynamic tile deal: every tile exactly once, whoever takes it
dbad = 0
chip = (ctypes.c_int32 * 2)()
if args.deal:
    # the chip the library plans with (the device's, or a forced CU count): persistent_grid is rounded down to a multiple of its
    # XCD count, and the case is sized from the grid that is left so that every workgroup walks >= 16 tiles on every chip
    _lib.check(_lib.lib().sicn_debug_chip(chip), "sicn_debug_chip")
for case in range(args.deal):
    tr = int(rng.integers(2))
    grid = max(int(rng.choice([8, 16])) // chip[1] * chip[1], chip[1])
    # position grid (output for the conv, input for the deconv) of tx x ty tiles of 16 x 32, ragged at both edges, with >= 16 tiles per workgroup
    n = int(rng.integers(1, 4))
    need = (16 * grid + n - 1) // n                      # tiles per image
    tx = int(rng.integers(2, 12))
    ty = max(1, (need + tx - 1) // tx + int(rng.integers(0, 3)))
    mw, mh = 32 * (tx - 1) + int(rng.integers(1, 33)), 16 * (ty - 1) + int(rng.integers(1, 17))
    assert ((mw + 31) // 32) * ((mh + 15) // 16) * n >= 16 * grid
    w, h = (mw, mh) if tr else (2 * mw - int(rng.integers(2)), 2 * mh - int(rng.integers(2)))
    d = LayerDesc.make(128, 128, 8, 16, w, h, tr)
    plan = (ctypes.c_int32 * 12)()
    _lib.check(_lib.lib().sicn_debug_plan(ctypes.byref(d.to_c()), n, ctypes.byref(_lib.make_options(wave_tile=128, persistent_grid=grid)),
                                          chip[0], plan), "sicn_debug_plan")
    assert (plan[1], plan[3], plan[7], plan[10]) == (chip[1], 2, grid, 1), list(plan)      # wide persistent, `grid` workgroups, dealt dynamically
    Wt = rng.integers(-8, 8, (128, 5, 5, 128)).astype(np.int8)
    bt = rng.integers(-128, 128, 128).astype(np.int8)
    fpw = api.FixedPointWeights(8, 4, 16, d.W_TILES, sicn_ref.pack_finn_tiles(Wt, 8, 16))
    net = api.EightLayersNet(descs=[d], params=[(fpw, api.FixedPointWeights(1, 8, 1, 128, bt.view(np.uint8).astype(np.uint64)))],
                             options={"wave_tile": 128, "persistent_grid": grid})
    x = rng.integers(0, 128, (n,) + d.in_shape, dtype=np.uint8)
    xin = torch.from_numpy(x).cuda()
    words = sicn_ref.pack_finn_tiles(Wt, 8, 16)
    ref = np.stack([c_oracle.run_layer(d, words, bt, x[i], form="direct", threads=THREADS) for i in range(n)])   # the C closed form: these are big
    ok = True
    out = None
    for _ in range(3):
        out, _ = net.run_layers(0, 0, xin)
        torch.cuda.synchronize()
        ok = ok and np.array_equal(out.cpu().numpy(), ref)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            net.run_layers(0, 0, xin, out=out)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        ok = ok and np.array_equal(out.cpu().numpy(), ref)
    if not ok:
        dbad += 1
        print(f"DEAL MISMATCH {case}: tr={tr} {w}x{h} n={n} grid={grid}", flush=True)
    else:
        print(f"deal {case}: ok ({'deconv' if tr else 'conv'} {w}x{h} n={n}, {grid} workgroups, {chip[1]} ticket counters)", flush=True)
if args.deal:
    print(f"{args.deal - dbad}/{args.deal} dynamic-deal cases bit-exact")
# the live-column kernels and the one-half layer 7: a producer that skips the accumulator columns its consumer does not read
lbad = 0
if args.live:
    import live_geometry_cases as lg  # noqa: E402  (next to this file)
    _lib.check(_lib.lib().sicn_debug_chip(chip), "sicn_debug_chip")
LIVE_COLUMNS = {112: 3, 96: 3, 80: 3, 79: 5, 48: 5, 47: 8, 0: 8}     # dead channels -> columns: 1 .. 3 run as 3, 4 and 5 as 5, 6 .. 8 as 8
for case in range(args.live):
    tr = int(rng.integers(2))
    kinds = ("deconv", "rgb" if rng.random() < 0.67 else "deconv") if tr else ("conv", "conv")
    tx, ty, n = int(rng.integers(1, 7)), int(rng.integers(1, 7)), int(rng.integers(1, 4))
    mw, mh = 32 * (tx - 1) + int(rng.integers(1, 33)), 16 * (ty - 1) + int(rng.integers(1, 17))      # ragged at both edges
    w, h = (mw, mh) if tr else (2 * mw - int(rng.integers(2)), 2 * mh - int(rng.integers(2)))
    grid = int(rng.choice([8, 16, 0]))
    grid = grid and max(grid // chip[1] * chip[1], chip[1])
    n_dead = int(rng.choice(list(LIVE_COLUMNS)))
    descs = lg.chain_descs(kinds, w, h)
    assert lg.tiles(descs[0]) == (tx, ty)
    wts = []
    for l, d in enumerate(descs):
        Wt = rng.integers(-8, 8, (d.OFM_CH, 5, 5, 128)).astype(np.int8)
        if l:
            Wt[:, :, :, rng.permutation(128)[:n_dead]] = 0
        wts.append((Wt, rng.integers(-128, 128, d.OFM_CH).astype(np.int8)))
    env = {"wave_tile": 128, "persistent_grid": grid}
    net = api.EightLayersNet(descs=descs, params=[(api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, lg.words(k, Wt)), bt)
                                                  for k, d, (Wt, bt) in zip(kinds, descs, wts)], options=env)
    cols, live = (ctypes.c_int32 * 2)(), (ctypes.c_int32 * 2)()
    _lib.check(_lib.lib().sicn_debug_net_columns(net._h, 0, 1, -1, n, cols, live), "sicn_debug_net_columns")
    assert (cols[0], cols[1], live[0]) == (LIVE_COLUMNS[n_dead], 8, 128 - n_dead), (list(cols), list(live), n_dead)
    x = rng.integers(0, 256, (n,) + descs[0].in_shape, dtype=np.uint8)
    ws = net.workspace(n)
    ws.copy_(torch.from_numpy(rng.integers(0, 256, ws.numel(), dtype=np.uint8)))       # positions nobody computes hold garbage
    out, _ = net.run_layers(0, 1, torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    ref = x
    for k, d, wb in zip(kinds, descs, wts):
        ref = lg.oracle_layer(k, d, wb, ref)
    what = f"{kinds[0]} {w}x{h} ({tx} x {ty} tiles) n={n} -> {kinds[1]}, grid {grid}, {n_dead} dead = {cols[0]} columns"
    if not np.array_equal(out.cpu().numpy(), ref):
        lbad += 1
        print(f"LIVE MISMATCH {case}: {what}", flush=True)
    elif case % 10 == 0:
        print(f"live {case}: ok ({what})", flush=True)
if args.live:
    print(f"{args.live - lbad}/{args.live} live-column cases bit-exact")
sys.exit(1 if (bad or cbad or gbad or dbad or lbad) else 0)
