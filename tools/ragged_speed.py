#!/usr/bin/env python3
"""Ragged batch against the ways the library could run a folder of differently sized images before it (profiles/ragged_batch_speed.txt).

A seeded mix of 64 image sizes, W and H each drawn from {256, 384, 512, 640, 768}, PARAM weights, whole 8-layer net with the latent:
  ragged   one RaggedNet call: 8 launches for the whole mix (the channel-generic MFMA kernels, csrc/k_ragged.hip; --rgb-ends
           packed | generic: the RGB ends on the packed-K kernels of csrc/k_ragged_rgb.hip or on the channel-generic ones;
           --rgb-layout interleaved | planar: the pixels as [h][w][3] or, include/sicn_ragged_planar.h, as [3][h][w] planes with the
           output written at the images' own sizes)
  loop     (a) one EightLayersNet per distinct size, created before timing, called once per image (the tuned kernels)
  grouped  (b) the same with the images of equal size grouped into one batch per size
  ceiling  the same number of pixels as ONE equal-size batch of 64 on the tuned kernels: what this untuned form is held to

Method: every shape is warmed up; then the variants ALTERNATE in one process for --rounds rounds, each timed with device events
around enough back-to-back repetitions to fill --seconds.  The outputs of ragged, loop and grouped are compared byte for byte in the
same run.  Verdict: ragged's median must be below both baselines' medians by more than the largest round-to-round spread (max - min
over the rounds) of any variant.

  python tools/ragged_speed.py                                  the table
  python tools/ragged_speed.py --only ragged --calls 20         just that variant, for a profiler run of its own:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ragged_speed.py --only ragged --calls 20
  python tools/ragged_speed.py --kernel-trace DIR/.../*_kernel_trace.csv     adds the per-layer table of that run
"""
import argparse
import csv
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

CHOICES = (256, 384, 512, 640, 768)


def make_sizes(seed, n):
    rng = np.random.default_rng(seed)
    return [(int(rng.choice(CHOICES)), int(rng.choice(CHOICES))) for _ in range(n)]


def per_layer_from_trace(path, calls_hint=None):
    """rocprofv3 kernel trace -> [(layer, kernel, mean us)] of the ragged kernels: dispatches in start order, 8 per forward call."""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    if not rows:
        return []
    key = {k.lower(): k for k in rows[0]}
    name, t0, t1 = key["kernel_name"], key["start_timestamp"], key["end_timestamp"]
    rows = sorted((r for r in rows if any(k in r[name] for k in ("k_any_ragged", "k_rgb_conv_ragged", "k_rgb_deconv_ragged"))),      # also *_planar
                  key=lambda r: int(r[t0]))
    rows = rows[len(rows) % 8:]                       # whole calls only
    out = []
    for l in range(8):
        mine = rows[l::8]
        if not mine:
            continue
        us = statistics.median((int(r[t1]) - int(r[t0])) / 1e3 for r in mine)
        out.append((l, mine[0][name].split("(")[0], us, len(mine)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rgb-ends", choices=["packed", "generic"], default="packed", help="the form of the ragged net's RGB ends")
    ap.add_argument("--rgb-layout", choices=["interleaved", "planar"], default="interleaved", help="the pixel layout of the ragged net's RGB boundaries")
    ap.add_argument("--only", choices=["ragged", "loop", "grouped", "ceiling"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernel-trace", help="a rocprofv3 *_kernel_trace.csv of an `--only ragged` run: print the per-layer table")
    ap.add_argument("--out", help="also write the table to this file")
    a = ap.parse_args()
    if a.rounds < 5 and not a.only:
        ap.error("--rounds: at least 5")

    import torch

    from simple_image_compression_network_amd import api
    from simple_image_compression_network_amd.config import eight_layer_descs

    sizes = make_sizes(a.seed, a.images)
    rng = np.random.default_rng(a.seed + 1)
    images = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for w, h in sizes]
    pixels = sum(w * h for w, h in sizes)
    weights = [api.DeviceWeights(d, w, b) for d, (w, b) in zip(eight_layer_descs(16, 16), api.load_param_weights())]

    # ---- the variants: every buffer is allocated before timing
    planar = a.rgb_layout == "planar"
    ragged = api.RaggedNet(sizes, shared_weights=weights, rgb_ends=a.rgb_ends, rgb_layout=a.rgb_layout)
    r_in = ragged.pack([x.permute(2, 0, 1) for x in images] if planar else images)
    r_out = torch.empty(ragged.nbytes(7), dtype=torch.uint8, device="cuda")
    r_lat = torch.empty(ragged.nbytes(3), dtype=torch.uint8, device="cuda")

    distinct = sorted(set(sizes))
    nets = {s: api.EightLayersNet(descs=eight_layer_descs(*s), shared_weights=weights) for s in distinct}
    l_in = [x[None] for x in images]
    l_out = [torch.empty((1,) + nets[s].descs[7].out_shape, dtype=torch.uint8, device="cuda") for s in sizes]
    l_lat = [torch.empty((1,) + nets[s].descs[3].out_shape, dtype=torch.uint8, device="cuda") for s in sizes]

    groups = {s: [i for i, t in enumerate(sizes) if t == s] for s in distinct}
    g_in = {s: torch.stack([images[i] for i in idx]) for s, idx in groups.items()}
    g_out = {s: torch.empty((len(idx),) + nets[s].descs[7].out_shape, dtype=torch.uint8, device="cuda") for s, idx in groups.items()}
    g_lat = {s: torch.empty((len(idx),) + nets[s].descs[3].out_shape, dtype=torch.uint8, device="cuda") for s, idx in groups.items()}

    edge = int(round((pixels / a.images) ** 0.5 / 16)) * 16
    c_net = api.EightLayersNet(descs=eight_layer_descs(edge, edge), shared_weights=weights)
    c_in = torch.from_numpy(rng.integers(0, 256, (a.images, edge, edge, 3), dtype=np.uint8)).cuda()
    c_out = torch.empty((a.images,) + c_net.descs[7].out_shape, dtype=torch.uint8, device="cuda")
    c_lat = torch.empty((a.images,) + c_net.descs[3].out_shape, dtype=torch.uint8, device="cuda")

    def run_ragged():
        ragged.forward(r_in, r_out, r_lat)

    def run_loop():
        for s, x, o, l in zip(sizes, l_in, l_out, l_lat):
            nets[s].forward(x, o, l)

    def run_grouped():
        for s in distinct:
            nets[s].forward(g_in[s], g_out[s], g_lat[s])

    def run_ceiling():
        c_net.forward(c_in, c_out, c_lat)

    variants = {"ragged": run_ragged, "loop": run_loop, "grouped": run_grouped, "ceiling": run_ceiling}
    if a.only:
        for _ in range(a.calls):
            variants[a.only]()
        torch.cuda.synchronize()
        print(f"{a.only}: {a.calls} calls done")
        return 0

    # ---- warm-up of every shape, then the equality of the three in this very run
    for fn in variants.values():
        fn()
        fn()
    torch.cuda.synchronize()
    r_outs, r_lats = ragged.views(7, r_out), ragged.views(3, r_lat)
    if planar:          # [3][h][w] at the image's size: the corner of the chain-rule reconstruction, permuted (these sizes are their own corner)
        r_outs = [v.permute(1, 2, 0) for v in r_outs]
    equal = True
    for i, s in enumerate(sizes):
        k = groups[s].index(i)
        h, w = r_outs[i].shape[:2]
        equal &= torch.equal(r_outs[i], l_out[i][0][:h, :w]) and torch.equal(r_lats[i], l_lat[i][0])
        equal &= torch.equal(r_outs[i], g_out[s][k][:h, :w]) and torch.equal(r_lats[i], g_lat[s][k])
    nonzero = float((r_lat != 0).float().mean())

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    reps = {k: max(2, int(a.seconds * 1e3 / timed(fn, 3)) + 1) for k, fn in variants.items()}
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, reps[k]))

    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    worst = max(spread.values())
    ok = equal and med["ragged"] + worst < med["loop"] and med["ragged"] + worst < med["grouped"]

    lines = []
    counts = {s: len(idx) for s, idx in groups.items()}
    lines.append(f"tools/ragged_speed.py --seed {a.seed} --images {a.images} --rounds {a.rounds} --seconds {a.seconds} --rgb-ends {a.rgb_ends}"
                 + (f" --rgb-layout {a.rgb_layout}" if planar else ""))
    lines.append("ragged kernels per layer: " + " ".join(ragged.kernel_for(l) for l in range(8)))
    lines.append(f"device: {torch.cuda.get_device_name(0)}; {a.images} images, {len(distinct)} distinct sizes, {pixels / 1e6:.2f} Mpixel in all; PARAM weights")
    lines.append("sizes W x H (count): " + ", ".join(f"{w}x{h} ({counts[(w, h)]})" for w, h in distinct))
    lines.append(f"outputs of ragged, loop and grouped byte-equal (reconstruction and latent of all {a.images} images): {equal}; "
                 f"non-zero latent bytes {nonzero:.2f}")
    lines.append("")
    lines.append(f"{'variant':<9}{'launches':>9}{'reps':>6}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'spread ms':>11}{'Mpixel/s':>10}   rounds (ms)")
    launches = {"ragged": 8, "loop": 8 * a.images, "grouped": 8 * len(distinct), "ceiling": 8}
    for k in variants:
        px = a.images * edge * edge if k == "ceiling" else pixels
        lines.append(f"{k:<9}{launches[k]:>9}{reps[k]:>6}{med[k]:>11.3f}{min(ms[k]):>9.3f}{max(ms[k]):>9.3f}{spread[k]:>11.3f}{px / med[k] / 1e3:>10.0f}   "
                     + " ".join(f"{v:.3f}" for v in ms[k]))
    lines.append(f"(ceiling: {a.images} x {edge} x {edge} = {a.images * edge * edge / 1e6:.2f} Mpixel as one equal-size batch on the tuned kernels)")
    lines.append("")
    lines.append(f"acceptance: median(ragged) + largest spread of any variant ({worst:.3f} ms) < median(loop) and < median(grouped): "
                 f"{med['ragged'] + worst:.3f} < {med['loop']:.3f} and < {med['grouped']:.3f} -> {'HOLDS' if ok else 'DOES NOT HOLD'}")
    lines.append(f"ragged / loop = {med['ragged'] / med['loop']:.2f}, ragged / grouped = {med['ragged'] / med['grouped']:.2f}, "
                 f"ragged / ceiling (per pixel) = {med['ragged'] / pixels / (med['ceiling'] / (a.images * edge * edge)):.2f}")
    if a.kernel_trace:
        lines.append("")
        lines.append(f"per layer, from a profiler run of its own (rocprofv3 --kernel-trace --stats -- tools/ragged_speed.py --only ragged): "
                     "median us per dispatch")
        total = 0.0
        for l, kern, us, n in per_layer_from_trace(a.kernel_trace):
            total += us
            items = _items(api, ragged, l)
            blocks = 1 if "_rgb_" in ragged.kernel_for(l) else (ragged.descs[l].OFM_CH + 63) // 64
            lines.append(f"  layer {l}  {us:9.1f} us  {items:7d} work items x {blocks} channel blocks  {kern}  ({n} dispatches)")
        lines.append(f"  sum      {total:9.1f} us of {med['ragged'] * 1e3:.1f} us per call measured above")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0 if equal else 2          # the verdict is a measurement, printed above; only unequal outputs are an error


def _items(api, net, layer):
    import ctypes
    q = (ctypes.c_int64 * 3)()
    api._lib.check(api._lib.lib().sicn_ragged_rgb_layout(net._cdescs, len(net.descs), net._widths, net._heights, len(net.sizes),
                                                         api._lib.RAGGED_RGB_ENDS[net.rgb_ends], layer, 0, q), "sicn_ragged_rgb_layout")
    return int(q[2])


if __name__ == "__main__":
    sys.exit(main())
