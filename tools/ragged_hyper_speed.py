#!/usr/bin/env python3
"""Ragged hyperprior codec against one uniform hyperprior codec per image (profiles/ragged_hyper_speed.txt).

The workload of tools/ragged_speed.py: the seeded mix of 64 image sizes, W and H each drawn from {256, 384, 512, 640, 768}, PARAM
weights in the main transform, seeded hyper stacks and GDN parameters; one step is encode + decode of the whole mix by
  ragged   one hyperprior.RaggedHyperpriorCodec: main transform, hyper stacks, both coders and the scale-map crop are per-BATCH launches
  loop     one hyperprior.HyperpriorCodec(w_i, h_i, 1) per image, created before timing, one encode + one decode call per image: every
           stage is per-image launches, on the tuned kernels of that size
Both use each image's own automatic z stream length, so the two write the same bytes.

Method: both variants are warmed up; then they ALTERNATE in one process for --rounds rounds, each timed with device events around
enough back-to-back repetitions to fill --seconds.  Containers and reconstructions are compared byte for byte in the same run.
There is NO acceptance ratio: the ragged layers are the untuned channel-generic kernels (profiles/ragged_batch_speed.txt) against the
tuned ones of each size; the table says what was measured.  (The y coder alone: tools/ragged_ctx_speed.py.)

  python tools/ragged_hyper_speed.py --out profiles/ragged_hyper_speed.txt
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from ragged_speed import make_sizes  # noqa: E402  (the same seeded mix)

# launches of one RaggedContextCoder call (csrc/k_ragged_ctx.hip): encode 6 kernels; decode 5 kernels + up to 2 k_ragged_ctx_decode + 1 memset node
CTX_ENC, CTX_DEC = 6, 8


def stage_launches(use_gdn=True):
    """[(stage, encode launches, decode launches, per)] of RaggedHyperpriorCodec, from the launch functions' own structure."""
    act = 3 if use_gdn else 0
    return [("main analysis, layers 0-3" + (" + 3 GDN" if use_gdn else ""), 4 + act, 0, "batch"),
            ("h_a, 2 layers", 2, 0, "batch"),
            ("z coder (ragged rANS-W)", 3, 2, "batch"),
            ("h_s, 2 layers", 2, 2, "batch"),
            ("scale-map crop", 1, 1, "batch"),
            ("main synthesis, layers 4-7" + (" + 3 IGDN" if use_gdn else ""), 0, 4 + act, "batch"),
            ("y coder (ragged rANS-WC)", CTX_ENC, CTX_DEC, "batch")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", help="also write the table to this file")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: at least 5")

    import numpy as np
    import torch

    from simple_image_compression_network_amd import api, hyperprior

    sizes = make_sizes(a.seed, a.images)
    rng = np.random.default_rng(a.seed + 1)
    images = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for w, h in sizes]
    pixels = sum(w * h for w, h in sizes)

    # ---- the variants: every buffer is allocated before timing
    params = api.load_param_weights()
    ragged = hyperprior.RaggedHyperpriorCodec(sizes, seed=a.seed, main_params=params)
    r_in = ragged.main.pack(images)
    r_out = torch.empty(ragged.main.nbytes(7), dtype=torch.uint8, device="cuda")

    loop = [hyperprior.HyperpriorCodec(w, h, 1, seed=a.seed, main_params=params) for w, h in sizes]
    l_in = [x[None].contiguous() for x in images]
    l_out = [torch.empty((1,) + c.main.descs[-1].out_shape, dtype=torch.uint8, device="cuda") for c in loop]

    def run_ragged():
        ragged.encode(r_in)
        ragged.decode(r_out)

    def run_loop():
        for c, x, out in zip(loop, l_in, l_out):
            c.encode(x)
            c.decode(out)

    variants = {"ragged": run_ragged, "loop": run_loop}

    # ---- warm-up, then the equality of the two in this very run
    for fn in variants.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ragged.check()
    r_cont = ragged.containers()
    equal = True
    for i, (c, v) in enumerate(zip(loop, ragged.main.views(7, r_out))):
        c.check()
        z = c.z_coder.slots[0, :c.z_coder.sizes()[0]].cpu().numpy().tobytes()
        y = c.y_coder.slots[0, :c.y_coder.sizes()[0]].cpu().numpy().tobytes()
        equal &= (z, y) == r_cont[i] and torch.equal(l_out[i][0], v)
    coded = sum(len(z) + len(y) for z, y in r_cont)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    reps = {k: max(2, int(a.seconds * 1e3 / timed(fn, 2)) + 1) for k, fn in variants.items()}
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, reps[k]))
    med = {k: statistics.median(v) for k, v in ms.items()}

    lines = []
    distinct = sorted(set(sizes))
    lines.append(f"tools/ragged_hyper_speed.py --seed {a.seed} --images {a.images} --rounds {a.rounds} --seconds {a.seconds}")
    lines.append(f"device: {torch.cuda.get_device_name(0)}; {a.images} images of {len(distinct)} distinct sizes, {pixels / 1e6:.2f} Mpixel; "
                 f"{coded / 1e6:.2f} MB coded, {8 * coded / pixels:.2f} bit / pixel")
    lines.append(f"containers (z and y) and reconstructions of ragged and loop byte-equal (all {a.images} images): {equal}")
    lines.append("")
    lines.append(f"{'variant':<9}{'reps':>6}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'spread ms':>11}{'Mpixel/s':>10}   rounds (ms), encode + decode")
    for k in variants:
        lines.append(f"{k:<9}{reps[k]:>6}{med[k]:>11.3f}{min(ms[k]):>9.3f}{max(ms[k]):>9.3f}{max(ms[k]) - min(ms[k]):>11.3f}{pixels / med[k] / 1e3:>10.0f}   "
                     + " ".join(f"{v:.3f}" for v in ms[k]))
    lines.append("")
    lines.append(f"ragged / loop = {med['ragged'] / med['loop']:.2f} (no acceptance ratio: the ragged layers are the untuned channel-generic kernels "
                 "against the tuned ones of each size)")
    lines.append("")
    lines.append("launches of one ragged step, per stage (from the launch functions; the y coder's decode includes its memset node):")
    lines.append(f"  {'stage':<52}{'encode':>8}{'decode':>8}   per")
    stages = stage_launches()
    for name, e, d, per in stages:
        lines.append(f"  {name:<52}{e:>8}{d:>8}   {per}")
    be, bd = (sum(s[i] for s in stages) for i in (1, 2))
    lines.append(f"  per batch: {be} + {bd}, whatever the number of images; the loop launches every stage once per image")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0 if equal else 2          # only unequal outputs are an error


if __name__ == "__main__":
    sys.exit(main())
