#!/usr/bin/env python3
"""Speed of conv2d<> / deconv522<> at channel widths the reference net does not instantiate: the default dispatch
(the channel-generic MFMA kernels, csrc/k_mfma16c.hip) against force_generic = 1 (k_generic, the kernel these shapes ran on before),
both in ONE process per shape, on one 1080p-derived grid; the MFMA side alone on the 8 x 4K-derived grid of layer 1 / layer 6; and the
software-pipelined 128 -> 128 kernels (prefetch = 2) on the same grids as the ceiling this untuned form is held against.

Device time per launch: one event pair around every launch, after warm-up launches; the median is reported (and every sample).
TOP/s = 2 x the layer's zero-skipped multiply-accumulates (LayerDesc.algorithmic_macs) / time.

Without --step this is only a driver: every step is a child process under its own time limit, and the first step that fails, faults
or runs out of time ends the run — nothing more is started on the GPU after it."""
import argparse
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# (cin, cout, simd, pe) of the inner layers; every one as a conv and as a deconv
INNER = [(64, 64, 8, 16), (192, 192, 12, 24), (256, 256, 8, 16), (192, 320, 8, 16), (320, 192, 16, 16)]
CEILING = (128, 128, 8, 16)
# 1080p-derived grid: layer 1 reads 960 x 540, layer 6 reads 480 x 270 (layer 0 reads 1920 x 1080, layer 7 reads 960 x 540)
CONV_IN, DECONV_IN, RGB_CONV_IN, RGB_DECONV_IN = (960, 540), (480, 270), (1920, 1080), (960, 540)
# 8 x 4K-derived grid of layer 1 / layer 6
BIG_CONV_IN, BIG_DECONV_IN, BIG_N = (1920, 1080), (960, 540), 8
GENERIC_LAUNCH_LIMIT_MS = 2000.0      # a k_generic launch slower than this: the shape is timed on a grid of half the height


def steps():
    out = []
    for (ci, co, simd, pe) in INNER:
        out.append((f"conv_{ci}_{co}", (ci, co, simd, pe, 0) + CONV_IN + (1, "both")))
        out.append((f"deconv_{ci}_{co}", (ci, co, simd, pe, 1) + DECONV_IN + (1, "both")))
    out.append(("conv_3_192", (3, 192, 3, 8, 0) + RGB_CONV_IN + (1, "both")))
    out.append(("deconv_192_3", (192, 3, 8, 3, 1) + RGB_DECONV_IN + (1, "both")))
    ci, co, simd, pe = CEILING
    out.append(("ceiling_conv_128_128", (ci, co, simd, pe, 0) + CONV_IN + (1, "pipelined")))
    out.append(("ceiling_deconv_128_128", (ci, co, simd, pe, 1) + DECONV_IN + (1, "pipelined")))
    for (ci, co, simd, pe) in INNER:
        out.append((f"big_conv_{ci}_{co}", (ci, co, simd, pe, 0) + BIG_CONV_IN + (BIG_N, "default")))
        out.append((f"big_deconv_{ci}_{co}", (ci, co, simd, pe, 1) + BIG_DECONV_IN + (BIG_N, "default")))
    ci, co, simd, pe = CEILING
    out.append(("big_ceiling_conv_128_128", (ci, co, simd, pe, 0) + BIG_CONV_IN + (BIG_N, "pipelined")))
    out.append(("big_ceiling_deconv_128_128", (ci, co, simd, pe, 1) + BIG_DECONV_IN + (BIG_N, "pipelined")))
    return out


def run_step(name):
    import ctypes

    import numpy as np
    import torch

    from simple_image_compression_network_amd import api
    from simple_image_compression_network_amd.config import LayerDesc
    from simple_image_compression_network_amd.hyperprior import random_layer_params

    ci, co, simd, pe, tr, w, h, n, mode = dict(steps())[name]
    rng = np.random.default_rng(0)

    def make(w, h):
        return LayerDesc.make(ci, co, simd, pe, w, h, tr)

    def timed(fn, warmup, reps):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return sorted(a.elapsed_time(b) for a, b in ev)

    d = make(w, h)
    (fw, fb), _ = random_layer_params(rng, d)
    dw = api.DeviceWeights(d, fw, fb)
    kernel = api._lib.lib().sicn_kernel_for(ctypes.byref(d.to_c())).decode()
    run = api.deconv522 if tr else api.conv2d
    while True:
        x = torch.from_numpy(rng.integers(0, 128, (n,) + d.in_shape, dtype=np.uint8)).cuda()
        out = torch.empty((n,) + d.out_shape, dtype=torch.uint8, device="cuda")
        slow = None
        if mode == "both":
            # the first k_generic launch doubles as its warm-up and decides whether the grid has to shrink
            ref = torch.empty_like(out)
            first = timed(lambda: run(d, dw, None, x, ref, n, options={"force_generic": 1}), 0, 1)[0]
            if first > GENERIC_LAUNCH_LIMIT_MS and d.IFM_COL > 32:
                print(f"# {name}: one k_generic launch took {first:.0f} ms on {d.IFM_ROW} x {d.IFM_COL}: halving the height")
                d = make(d.IFM_ROW, d.IFM_COL // 2)
                continue
            slow = timed(lambda: run(d, dw, None, x, ref, n, options={"force_generic": 1}), 0, 3)
        break
    opts = {"prefetch": 2} if mode == "pipelined" else None
    fast = timed(lambda: run(d, dw, None, x, out, n, options=opts), 3, 20)
    ops = 2.0 * n * d.algorithmic_macs
    med = fast[len(fast) // 2]
    line = (f"{name:28s} {'deconv' if tr else 'conv  '} {ci:4d} -> {co:4d}  in {n} x {d.IFM_ROW} x {d.IFM_COL}  "
            f"{kernel + (' prefetch=2' if opts else ''):22s} {med * 1e3:10.1f} us  {ops / med / 1e9:8.2f} TOP/s  "
            f"(min {fast[0] * 1e3:.1f}, max {fast[-1] * 1e3:.1f}, 20 launches)")
    if slow is not None:
        smed = slow[len(slow) // 2]
        line += (f" | generic {smed * 1e3:12.1f} us  {ops / smed / 1e9:7.3f} TOP/s  ({', '.join(f'{v * 1e3:.0f}' for v in slow)} us)"
                 f" | x{smed / med:7.1f} | bytes equal: {torch.equal(out, ref)}")
    print(line, flush=True)
    if slow is not None and not torch.equal(out, ref):
        return 1
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--step", help="run one step in this process (what the driver starts)")
    ap.add_argument("--only", help="comma-separated step names, or a prefix ending in '*'")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        return run_step(a.step)
    names = [s for s, _ in steps()]
    if a.only:
        want = a.only.split(",")
        names = [s for s in names if any(s == o or (o.endswith("*") and s.startswith(o[:-1])) for o in want)]
    print("# tools/any_width_speed.py: median device time per launch (one event pair per launch, 3 warm-up + 20 launches; k_generic: "
          "1 + 3 launches); TOP/s = 2 x zero-skipped MACs / time; 'x' = generic / default", flush=True)
    for s in names:
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--step", s], timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"# {s}: no result after {a.step_timeout} s; stopping here", flush=True)
            return 124
        if r.returncode != 0:
            print(f"# {s}: exit status {r.returncode} after {time.time() - t0:.0f} s; stopping here", flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
