#!/usr/bin/env python3
"""Ragged context coder against the ways the library could code the y latents of a ragged hyperprior batch before it
(profiles/ragged_ctx_speed.txt).

The workload of tools/ragged_hyper_speed.py: the seeded mix of 64 image sizes, W and H each drawn from {256, 384, 512, 640, 768}; its
latents and scale maps — hyperprior.RaggedHyperpriorCodec's `y` and `s`, made once, before timing — are encoded AND decoded by
  ragged   one codec.RaggedContextCoder: 6 + 8 launches for the whole mix (csrc/k_ragged_ctx.hip)
  loop     one codec.ContextCoder(1, ...) per image, created before timing, one encode + one decode call per image: 64 x (8 + 8) launches
  grouped  one codec.ContextCoder(k, ...) per distinct size with the k images of that size as one batch: 8 + 8 launches per size
(the decoders' launch counts include their memset node).  The three write the same bytes.

Method: every shape is warmed up; then the variants ALTERNATE in one process for --rounds rounds, each timed with device events
around enough back-to-back repetitions to fill --seconds.  Containers and decoded latents of the three are compared byte for byte in
the same run.  Verdict: ragged's median must be below both baselines' medians by more than the largest round-to-round spread (max -
min over the rounds) of any variant.

  python tools/ragged_ctx_speed.py                                  the table
  python tools/ragged_ctx_speed.py --only ragged --images 1 --calls 20       just that variant, for a profiler run of its own:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ragged_ctx_speed.py --only ragged --images 1 --calls 20
  python tools/ragged_ctx_speed.py --count-trace DIR/.../*_kernel_trace.csv --calls 20       the dispatches per encode and per decode of that run
"""
import argparse
import csv
import re
import statistics
import sys
from collections import Counter
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from ragged_speed import make_sizes  # noqa: E402  (the same seeded mix)

ENC_KERNELS = ("clear", "stats<true>", "tables", "encode", "scan", "compact")            # tables and scan run in both directions
DEC_KERNELS = ("parse", "tables", "scan", "decode<0>", "decode<1>", "stats<false>", "finish")


def launches_from_trace(path):
    """rocprofv3 kernel trace -> Counter of the ragged context coder's kernels by name (namespace and signature dropped, the template
    argument kept: k_ragged_ctx_stats<true> is the encoder's, <false> the decoder's)."""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    if not rows:
        return Counter()
    name = {k.lower(): k for k in rows[0]}["kernel_name"]
    found = (re.search(r"\bk_ragged_ctx_[a-z_]+(?:<[a-z0-9]+>)?", r[name]) for r in rows)
    return Counter(m.group(0) if m else "(other: the runtime's fill kernel of the memset node, the workload's set-up)" for m in found)


def count_trace(path, calls):
    """Dispatches per encode and per decode of an `--only ragged --calls N` run.  tables and scan run once in either direction."""
    found = launches_from_trace(path)
    lines = [f"  {kern:<28}{cnt:6d} dispatches = {cnt / calls:.2f} per encode + decode" for kern, cnt in sorted(found.items())]
    both = sum(found[f"k_ragged_ctx_{k}"] for k in ("tables", "scan")) / 2
    enc = sum(found[f"k_ragged_ctx_{k}"] for k in ENC_KERNELS if k not in ("tables", "scan")) + both
    dec = sum(found[f"k_ragged_ctx_{k}"] for k in DEC_KERNELS if k not in ("tables", "scan")) + both
    lines.append(f"  kernel dispatches per encode: {enc / calls:.2f}; per decode: {dec / calls:.2f} (+ 1 memset node, which the kernel trace does not list)")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--only", choices=["ragged", "loop", "grouped"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--count-trace", help="a rocprofv3 *_kernel_trace.csv of an `--only ragged --calls N` run: print its launch counts and exit")
    ap.add_argument("--out", help="also write the table to this file")
    a = ap.parse_args()
    if a.count_trace:
        print(count_trace(a.count_trace, a.calls))
        return 0
    if a.rounds < 5 and not a.only:
        ap.error("--rounds: at least 5")

    import numpy as np
    import torch

    from simple_image_compression_network_amd import api, codec, hyperprior

    sizes = make_sizes(a.seed, a.images)
    rng = np.random.default_rng(a.seed + 1)
    images = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for w, h in sizes]
    hc = hyperprior.RaggedHyperpriorCodec(sizes, seed=a.seed, main_params=api.load_param_weights())
    hc.main.run_layers(0, 3, hc.main.pack(images), out=hc.y)    # encode() without its coders (so that a profiler run of --only
    hc.h_a.run_layers(0, 1, hc.y, out=hc.z)                     # sees the calls below and no others): y, z, and s = crop(h_s(z))
    hc._scale_map(hc.z)
    torch.cuda.synchronize()
    r_y, r_s = hc.y.clone(), hc.s.clone()                       # the workload: made once
    shapes = hc.main.shapes(3)                                   # (h, w, c) per image
    y_views, s_views = hc.main.views(3, r_y), hc.main.views(3, r_s)
    symbols = sum(h * w * c for h, w, c in shapes)
    del hc

    # ---- the variants: every buffer is allocated before timing
    ragged = codec.RaggedContextCoder([(h, w) for h, w, _ in shapes], shapes[0][2], sizes)
    r_back = torch.empty_like(r_y)

    loop = [codec.ContextCoder(1, h, w, c, iw, ih) for (h, w, c), (iw, ih) in zip(shapes, sizes)]
    l_y, l_s = [v[None].contiguous() for v in y_views], [v[None].contiguous() for v in s_views]
    l_back = [torch.empty_like(x) for x in l_y]

    distinct = sorted(set(sizes))
    groups = {s: [i for i, t in enumerate(sizes) if t == s] for s in distinct}
    grouped = {s: codec.ContextCoder(len(idx), *shapes[idx[0]], s[0], s[1]) for s, idx in groups.items()}
    g_y = {s: torch.stack([y_views[i] for i in idx]).contiguous() for s, idx in groups.items()}
    g_s = {s: torch.stack([s_views[i] for i in idx]).contiguous() for s, idx in groups.items()}
    g_back = {s: torch.empty_like(x) for s, x in g_y.items()}

    def run_ragged():
        ragged.encode(r_y, r_s)
        ragged.decode(r_back, r_s)

    def run_loop():
        for coder, y, s, back in zip(loop, l_y, l_s, l_back):
            coder.encode(y, s)
            coder.decode(back, s)

    def run_grouped():
        for k in distinct:
            grouped[k].encode(g_y[k], g_s[k])
            grouped[k].decode(g_back[k], g_s[k])

    variants = {"ragged": run_ragged, "loop": run_loop, "grouped": run_grouped}
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
    ragged.check()
    r_cont = ragged.containers()
    equal = torch.equal(r_back, r_y)
    for i, s in enumerate(sizes):
        k = groups[s].index(i)
        loop[i].check()
        one = loop[i].slots[0, :loop[i].sizes()[0]].cpu().numpy().tobytes()
        grp = grouped[s].slots[k, :grouped[s].sizes()[k]].cpu().numpy().tobytes()
        equal &= one == r_cont[i] and grp == r_cont[i]
        equal &= torch.equal(l_back[i][0], y_views[i]) and torch.equal(g_back[s][k], y_views[i])
    coded = sum(len(c) for c in r_cont)

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
    streams = sum(int(im.anchor_streams) + int(im.nonanchor_streams) for im in ragged.images[:a.images])
    lines.append(f"tools/ragged_ctx_speed.py --seed {a.seed} --images {a.images} --rounds {a.rounds} --seconds {a.seconds}")
    lines.append(f"device: {torch.cuda.get_device_name(0)}; {a.images} latents of {len(distinct)} distinct shapes, {symbols / 1e6:.2f} M symbols in "
                 f"{streams} streams; {coded / 1e6:.2f} MB coded, {8 * coded / symbols:.2f} bit / symbol")
    lines.append("image sizes W x H (count): " + ", ".join(f"{w}x{h} ({counts[(w, h)]})" for w, h in distinct))
    lines.append(f"containers and decoded latents of ragged, loop and grouped byte-equal (all {a.images} images): {equal}")
    lines.append("")
    lines.append(f"{'variant':<9}{'launches':>9}{'reps':>6}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'spread ms':>11}{'Msymbol/s':>11}   rounds (ms), encode + decode")
    launches = {"ragged": 14, "loop": 16 * a.images, "grouped": 16 * len(distinct)}
    for k in variants:
        lines.append(f"{k:<9}{launches[k]:>9}{reps[k]:>6}{med[k]:>11.3f}{min(ms[k]):>9.3f}{max(ms[k]):>9.3f}{spread[k]:>11.3f}{symbols / med[k] / 1e3:>11.0f}   "
                     + " ".join(f"{v:.3f}" for v in ms[k]))
    lines.append("")
    lines.append(f"acceptance: median(ragged) + largest spread of any variant ({worst:.3f} ms) < median(loop) and < median(grouped): "
                 f"{med['ragged'] + worst:.3f} < {med['loop']:.3f} and < {med['grouped']:.3f} -> {'HOLDS' if ok else 'DOES NOT HOLD'}")
    lines.append(f"ragged / loop = {med['ragged'] / med['loop']:.2f}, ragged / grouped = {med['ragged'] / med['grouped']:.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0 if equal else 2          # the verdict is a measurement, printed above; only unequal outputs are an error


if __name__ == "__main__":
    sys.exit(main())
