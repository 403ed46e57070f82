#!/usr/bin/env python3
"""Ragged latent coder against the ways the library could code the latents of a ragged batch before it (profiles/ragged_coder_speed.txt).

The workload of tools/ragged_speed.py: the seeded mix of 64 image sizes, W and H each drawn from {256, 384, 512, 640, 768}, PARAM
weights; its boundary-3 latents (one RaggedNet call, before timing) are encoded AND decoded by
  ragged   one codec.RaggedLatentCoder: 3 + 2 launches for the whole mix (csrc/k_ragged_codec.hip)
  loop     one codec.LatentCoder(1, ...) per image, created before timing, one encode + one decode call per image: 64 x (3 + 2) launches
  grouped  one codec.LatentCoder(k, ...) per distinct size with the k images of that size as one batch: 3 + 2 launches per size
Every variant uses each image's own automatic stream length (codec.auto_stream_symbols), so the three write the same bytes.

Method: every shape is warmed up; then the variants ALTERNATE in one process for --rounds rounds, each timed with device events
around enough back-to-back repetitions to fill --seconds.  Containers and decoded latents of the three are compared byte for byte in
the same run.  Verdict: ragged's median must be below both baselines' medians by more than the largest round-to-round spread (max -
min over the rounds) of any variant.

  python tools/ragged_coder_speed.py                                the table
  python tools/ragged_coder_speed.py --only ragged --calls 20       just that variant, for a profiler run of its own:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ragged_coder_speed.py --only ragged --calls 20
  python tools/ragged_coder_speed.py --kernel-trace DIR/.../*_kernel_trace.csv --calls 20    adds the launch count of that run
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


def launches_from_trace(path):
    """rocprofv3 kernel trace -> Counter of the ragged coder's kernels by name (namespace, template arguments and signature dropped)."""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    if not rows:
        return Counter()
    name = {k.lower(): k for k in rows[0]}["kernel_name"]
    found = (re.search(r"\bk_ragged_(?:stats|encode|compact|decode|dec_finish)\b", r[name]) for r in rows)
    return Counter(m.group(0) for m in found if m)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--only", choices=["ragged", "loop", "grouped"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernel-trace", help="a rocprofv3 *_kernel_trace.csv of an `--only ragged --calls N` run: print its launch counts")
    ap.add_argument("--out", help="also write the table to this file")
    a = ap.parse_args()
    if a.rounds < 5 and not a.only:
        ap.error("--rounds: at least 5")

    import numpy as np
    import torch

    from simple_image_compression_network_amd import api, codec
    from simple_image_compression_network_amd.config import eight_layer_descs

    sizes = make_sizes(a.seed, a.images)
    rng = np.random.default_rng(a.seed + 1)
    images = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for w, h in sizes]
    weights = [api.DeviceWeights(d, w, b) for d, (w, b) in zip(eight_layer_descs(16, 16), api.load_param_weights())]
    net = api.RaggedNet(sizes, shared_weights=weights)
    r_lat, _ = net.run_layers(0, 3, net.pack(images))
    torch.cuda.synchronize()
    lat_views = net.views(3, r_lat)
    shapes = net.shapes(3)                                      # (h, w, c) per image
    symbols = sum(h * w * c for h, w, c in shapes)

    # ---- the variants: every buffer is allocated before timing
    ragged = net.latent_coder()
    r_back = torch.empty_like(r_lat)

    loop = [codec.LatentCoder(1, h, w, c, iw, ih) for (h, w, c), (iw, ih) in zip(shapes, sizes)]
    l_in = [v[None].contiguous() for v in lat_views]
    l_back = [torch.empty_like(x) for x in l_in]

    distinct = sorted(set(sizes))
    groups = {s: [i for i, t in enumerate(sizes) if t == s] for s in distinct}
    grouped = {s: codec.LatentCoder(len(idx), *shapes[idx[0]], s[0], s[1]) for s, idx in groups.items()}
    g_in = {s: torch.stack([lat_views[i] for i in idx]).contiguous() for s, idx in groups.items()}
    g_back = {s: torch.empty_like(x) for s, x in g_in.items()}

    def run_ragged():
        ragged.encode(r_lat)
        ragged.decode(r_back)

    def run_loop():
        for coder, x, back in zip(loop, l_in, l_back):
            coder.encode(x)
            coder.decode(back)

    def run_grouped():
        for s in distinct:
            grouped[s].encode(g_in[s])
            grouped[s].decode(g_back[s])

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
    equal = torch.equal(r_back, r_lat)
    for i, s in enumerate(sizes):
        k = groups[s].index(i)
        loop[i].check()
        one = loop[i].slots[0, :loop[i].sizes()[0]].cpu().numpy().tobytes()
        grp = grouped[s].slots[k, :grouped[s].sizes()[k]].cpu().numpy().tobytes()
        equal &= one == r_cont[i] and grp == r_cont[i]
        equal &= torch.equal(l_back[i][0], lat_views[i]) and torch.equal(g_back[s][k], lat_views[i])
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
    streams = sum(int(im.n_streams) for im in ragged.images[:a.images])
    lines.append(f"tools/ragged_coder_speed.py --seed {a.seed} --images {a.images} --rounds {a.rounds} --seconds {a.seconds}")
    lines.append(f"device: {torch.cuda.get_device_name(0)}; {a.images} latents of {len(distinct)} distinct shapes, {symbols / 1e6:.2f} M symbols in "
                 f"{streams} streams (stream lengths {sorted(set(ragged.stream_symbols))}); {coded / 1e6:.2f} MB coded, {8 * coded / symbols:.2f} bit / symbol")
    lines.append("image sizes W x H (count): " + ", ".join(f"{w}x{h} ({counts[(w, h)]})" for w, h in distinct))
    lines.append(f"containers and decoded latents of ragged, loop and grouped byte-equal (all {a.images} images): {equal}")
    lines.append("")
    lines.append(f"{'variant':<9}{'launches':>9}{'reps':>6}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'spread ms':>11}{'Msymbol/s':>11}   rounds (ms), encode + decode")
    launches = {"ragged": 5, "loop": 5 * a.images, "grouped": 5 * len(distinct)}
    for k in variants:
        lines.append(f"{k:<9}{launches[k]:>9}{reps[k]:>6}{med[k]:>11.3f}{min(ms[k]):>9.3f}{max(ms[k]):>9.3f}{spread[k]:>11.3f}{symbols / med[k] / 1e3:>11.0f}   "
                     + " ".join(f"{v:.3f}" for v in ms[k]))
    lines.append("")
    lines.append(f"acceptance: median(ragged) + largest spread of any variant ({worst:.3f} ms) < median(loop) and < median(grouped): "
                 f"{med['ragged'] + worst:.3f} < {med['loop']:.3f} and < {med['grouped']:.3f} -> {'HOLDS' if ok else 'DOES NOT HOLD'}")
    lines.append(f"ragged / loop = {med['ragged'] / med['loop']:.2f}, ragged / grouped = {med['ragged'] / med['grouped']:.2f}")
    if a.kernel_trace:
        lines.append("")
        lines.append(f"launches, from a profiler run of its own (rocprofv3 --kernel-trace --stats --output-format csv -- tools/ragged_coder_speed.py --only ragged "
                     f"--calls {a.calls}):")
        found = launches_from_trace(a.kernel_trace)
        for kern, cnt in sorted(found.items()):
            lines.append(f"  {kern:<24}{cnt:6d} dispatches = {cnt / a.calls:.2f} per encode + decode")
        lines.append(f"  {'all':<24}{sum(found.values()):6d} dispatches = {sum(found.values()) / a.calls:.2f} per encode + decode (3 + 2 expected)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0 if equal else 2          # the verdict is a measurement, printed above; only unequal outputs are an error


if __name__ == "__main__":
    sys.exit(main())
