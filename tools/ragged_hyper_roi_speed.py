#!/usr/bin/env python3
"""A 256 x 256 detail of a few images out of a device-resident ragged HYPERPRIOR archive: the ROI path of library 0.13 against the
only way before it, the full decode of the same images, the crop and a slice (profiles/ragged_hyper_roi_speed.txt).

The workload of tools/ragged_roi_speed.py in the hyperprior configuration: the seeded mix of 64 image sizes, PARAM weights for the
main transform, one archive (sections z and y) of all of them, already in device memory, and the selections {3, 17, 40, 63} and {17}.
The rectangle is 256 x 256, centred, clipped to the image.  For a selection, on objects made before timing:
  full   RaggedHyperpriorCodec.decode(archive=, images=) + main.cropped + the rectangle sliced out of every image (a view and one
         copy per image)
  roi    RaggedHyperpriorRoi.decode(archive=, images=): unpack, the z coder and h_s with its crop IN FULL, the window decoder over the
         y streams that hold the latent rows, the cut of the latent columns, layers 4-7 with IGDN over the windows, the cut of the
         rectangle
Both end with the device idle and are timed with the host's clock.

Method: both variants are warmed up; then they ALTERNATE in one process for --rounds rounds, each timed around enough back-to-back
repetitions to fill --seconds.  In every round the ROI bytes of both must be equal.  There is no ratio to meet: the table records
the times and the largest round-to-round spread (max - min over the rounds), and says whether the ROI path was faster.

  python tools/ragged_hyper_roi_speed.py                                    the table
  python tools/ragged_hyper_roi_speed.py --only roi --select 4 --calls 20   RaggedHyperpriorRoi.decode alone (--only full: the other),
      for a profiler run of its own:  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ragged_hyper_roi_speed.py --only roi ...
  python tools/ragged_hyper_roi_speed.py --kernel-trace roi:4=PATH --kernel-trace roi:1=PATH ... --calls 20 [--trace-only]
      adds the dispatch counts and device times of those runs (WHAT:SELECTED=path of the *_kernel_trace.csv), and the share of the
      stages that run in full (z coder, h_s, its crop) in the ROI path's device time
"""
import argparse
import csv
import re
import statistics
import sys
import time
from collections import defaultdict
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import roi_direct  # noqa: E402  (--roi-layout, --direct, --permute and the timed --only run)
from ragged_speed import make_sizes  # noqa: E402  (the same seeded mix)

SELECTIONS = {4: [3, 17, 40, 63], 1: [17]}
SIDE = 256
FIRST_KERNEL = "k_archive_parse"          # every call begins with the unpack of the archive (k_archive_parse_select)


def centred(size):
    w, h = size
    rw, rh = min(SIDE, w), min(SIDE, h)
    return ((w - rw) // 2, (h - rh) // 2, rw, rh)


def calls_from_trace(path, n_calls):
    """rocprofv3 kernel trace -> the LAST n_calls calls, each a list of (kernel, device ns) in time order.  A call begins at a
    dispatch of the unpack's first kernel; the warm-up calls in front of the timed ones are cut off by counting from the end."""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    if not rows:
        return []
    col = {k.lower(): k for k in rows[0]}
    rows.sort(key=lambda r: int(r[col["start_timestamp"]]))
    calls = []
    for r in rows:
        full = r[col["kernel_name"]]
        m = re.search(r"\b(k_[a-z0-9_]+)(<[^>]*>)?", full)
        name = (m.group(1) + (m.group(2) or "")) if m else "(runtime) " + full[:48]
        if name.startswith(FIRST_KERNEL):
            calls.append([])
        if calls:
            calls[-1].append((name, int(r[col["end_timestamp"]]) - int(r[col["start_timestamp"]])))
    calls = calls[-n_calls:]

    def tail(call):                                             # dispatches behind the library's last kernel
        return next((i for i, (k, _) in enumerate(reversed(call)) if not k.startswith("(runtime)")), len(call))
    if len(calls) > 1 and tail(calls[-1]) > tail(calls[-2]):    # the read-back of the final check(): torch's copies, not the call's
        calls[-1] = calls[-1][:len(calls[-1]) - (tail(calls[-1]) - tail(calls[-2]))]
    return calls


def stage_of(call, pos):
    """The stage of dispatch `pos` of one call of the ROI path.  In dispatch order the first cut is the crop of h_s, and the layer
    kernels in front of it are h_s's."""
    kernel = call[pos][0]
    first_cut = next((i for i, (k, _) in enumerate(call) if k.startswith("k_ragged_cut")), len(call))
    if kernel.startswith("k_archive"):
        return "unpack"
    if kernel.startswith("k_ragged_ctx"):
        return "y window decoder"
    if kernel.startswith("(runtime)"):
        return "y window decoder" if pos > first_cut else "other"          # the memset of the band tensor
    if kernel.startswith(("k_ragged_decode", "k_ragged_dec_finish")):
        return "z coder (full)"
    if kernel.startswith("k_ragged_cut"):
        return "crop of h_s (full)" if pos == first_cut else "latent and pixel cuts"
    return "h_s (full)" if pos < first_cut else "layers 4-7 and IGDN (windows)"


def trace_lines(specs, n_calls):
    lines, counts = [], {}
    for spec in specs:
        what, _, path = spec.partition("=")
        kind, _, selected = what.partition(":")
        lines.append("")
        lines.append(f"kernels of {n_calls} calls, {selected} image(s), from a profiler run of its own with nothing else in it (rocprofv3 "
                     f"--kernel-trace --stats --output-format csv -- tools/ragged_hyper_roi_speed.py --only {kind} --select {selected} --calls {n_calls}):")
        calls = calls_from_trace(path, n_calls)
        n = max(len(calls), 1)
        per_kernel, per_stage = defaultdict(list), defaultdict(float)
        for call in calls:
            for pos, (name, ns) in enumerate(call):
                per_kernel[name].append(ns)
                if kind == "roi":
                    per_stage[stage_of(call, pos)] += ns
        for kern, ns in per_kernel.items():
            lines.append(f"  {kern:<52}{len(ns):6d} dispatches = {len(ns) / n:.2f} per call, median {statistics.median(ns) / 1e3:.2f} us "
                         f"(min {min(ns) / 1e3:.2f}, max {max(ns) / 1e3:.2f}), {sum(ns) / n / 1e3:.2f} us per call")
        total = sum(len(v) for v in per_kernel.values())
        device = sum(sum(v) for v in per_kernel.values())
        per_call = sorted({len(c) for c in calls})
        counts[kind, selected] = per_call
        lines.append(f"  {'all':<52}{total:6d} dispatches in {len(calls)} calls, {per_call} per call, {device / n / 1e3:.2f} us of device time per call")
        for st, ns in per_stage.items():
            lines.append(f"    {st:<40}{ns / n / 1e3:9.2f} us per call = {100.0 * ns / device:5.1f} % of the device time")
        if per_stage:
            share = sum(ns for st, ns in per_stage.items() if "(full)" in st)
            lines.append(f"    the stages run in FULL (z coder, h_s, its crop): {100.0 * share / device:.1f} % of the ROI path's device time")
    for kind in ["roi"]:                                        # (the full variant slices with one copy per image)
        got = {sel: c for (k, sel), c in counts.items() if k == kind}
        if len(got) > 1:
            same = len({tuple(c) for c in got.values()}) == 1 and all(len(c) == 1 for c in got.values())
            lines.append("")
            lines.append(f"dispatches per call of `{kind}` by number of images: {got}: " +
                         ("EQUAL, whatever the number of images" if same else "NOT equal"))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--only", choices=["roi", "full"])
    ap.add_argument("--select", type=int, choices=sorted(SELECTIONS), default=4, help="with --only: the selection's size")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernel-trace", action="append", default=[], metavar="WHAT:SELECTED=PATH")
    ap.add_argument("--trace-only", action="store_true", help="print the --kernel-trace sections alone (no device needed)")
    ap.add_argument("--out", help="also write the table to this file")
    roi_direct.add_arguments(ap)
    a = ap.parse_args()
    roi_direct.check(ap, a)
    if a.rounds < 5 and not a.only:
        ap.error("--rounds: at least 5")
    if a.trace_only:
        print("\n".join(trace_lines(a.kernel_trace, a.calls)).lstrip("\n"))
        return 0

    import numpy as np
    import torch

    from simple_image_compression_network_amd import api, hyperprior

    sizes = make_sizes(a.seed, a.images)
    rng = np.random.default_rng(a.seed + 1)
    images = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in sizes]
    params = api.load_param_weights()
    whole = hyperprior.RaggedHyperpriorCodec(sizes, seed=a.seed, main_params=params)
    whole.encode(whole.main.pack(images))
    b = whole.archive()
    torch.cuda.synchronize()
    resident = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    del whole, images

    class Case:
        """One selection: its codec and RaggedHyperpriorRoi, all made before timing."""

        def __init__(self, sel):
            self.sel = sel
            self.codec = hyperprior.RaggedHyperpriorCodec.from_archive(b, seed=a.seed, main_params=params, images=sel)
            self.rects = [centred(s) for s in self.codec.sizes]
            self.index = torch.tensor(sel, dtype=torch.int32, device="cuda")
            self.roi = self.codec.roi(self.rects, **roi_direct.keywords(a))
            main = self.codec.main
            self.out = torch.empty(main.nbytes(7), dtype=torch.uint8, device="cuda")
            self.pixels = torch.empty(sum(3 * r[2] * r[3] for r in self.rects), dtype=torch.uint8, device="cuda")
            main.cropped(self.out)                                   # makes the crop object
            self.variants = {"full": self.full, "roi": self.by_roi}
            win = self.roi.window
            self.streams = (win.selected_streams, sum(int(im.anchor_streams) + int(im.nonanchor_streams) for im in self.codec.y_coder.images[:len(sel)]))
            self.band_rows = (sum(int(im.band_rows) for im in win.images[:len(sel)]), sum(p["rh"] for p in self.roi.plans),
                              sum(h for h, _, _ in main.shapes(3)))
            self.latent_positions = (sum(p["cw"] * p["rh"] for p in self.roi.plans), sum(h * w for h, w, _ in main.shapes(3)))
            self.pixel_counts = (sum(256 * p["cw"] * p["rh"] for p in self.roi.plans), sum(h * w for h, w, _ in main.shapes(7)),
                                 sum(r[2] * r[3] for r in self.rects))

        def full(self):
            main = self.codec.main
            out = self.codec.decode(out=self.out, archive=resident, images=self.index)
            views = main.crop_views(main.cropped(out))
            got = torch.cat([v[y0:y0 + h, x0:x0 + w].reshape(-1) for v, (x0, y0, w, h) in zip(views, self.rects)])
            torch.cuda.synchronize()
            return got

        def by_roi(self):
            got = self.roi.decode(archive=resident, images=self.index, out=self.pixels)
            torch.cuda.synchronize()
            return got

        def verify(self):
            self.pixels.zero_()
            a_ = self.by_roi().clone()
            self.roi.check()
            b_ = self.full()
            self.codec.check()
            return bool(torch.equal(a_, b_))

    if a.only:
        case = Case(SELECTIONS[a.select])
        fn = case.variants[a.only]
        fn()                                                         # warm-up: module load, first-use objects
        torch.cuda.synchronize()
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        (case.roi if a.only == "roi" else case.codec).check()
        if a.only == "roi":
            roi_direct.timed_only(a, "ragged_hyper_roi", lambda: case.roi.decode(archive=resident, images=case.index, out=case.pixels),
                                  case.roi.views)
        print(f"{a.only}: {a.calls} calls done, {len(case.sel)} of {len(sizes)} images")
        return 0

    cases = {n: Case(sel) for n, sel in SELECTIONS.items()}
    equal = True
    for case in cases.values():
        for fn in list(case.variants.values()) * 2:
            fn()
        equal &= case.verify()

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    ms, reps = {}, {}
    for n, case in cases.items():
        for k, fn in case.variants.items():
            reps[n, k] = max(2, int(a.seconds * 1e3 / timed(fn, 3)) + 1)
            ms[n, k] = []
    for _ in range(a.rounds):
        for (n, k) in ms:
            ms[n, k].append(timed(cases[n].variants[k], reps[n, k]))
        for case in cases.values():
            equal &= case.verify()

    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    lines = []
    lines.append(f"tools/ragged_hyper_roi_speed.py --seed {a.seed} --images {a.images} --rounds {a.rounds} --seconds {a.seconds}")
    lines.append(f"device: {torch.cuda.get_device_name(0)}; a hyperprior archive of {len(sizes)} images, {len(b)} bytes, resident in device memory; "
                 f"a centred {SIDE} x {SIDE} rectangle, clipped to the image")
    for n, case in cases.items():
        lines.append(f"{n} selected: images {case.sel}, sizes {case.codec.sizes}, rectangles {case.rects}")
        lines.append(f"   y streams selected / total {case.streams[0]} / {case.streams[1]}; latent rows in the bands / asked for / in the images "
                     f"{case.band_rows[0]} / {case.band_rows[1]} / {case.band_rows[2]}; latent positions in the windows / in the images "
                     f"{case.latent_positions[0]} / {case.latent_positions[1]}; pixels asked for {case.pixel_counts[2]}, synthesised by the ROI "
                     f"path {case.pixel_counts[0]}, by the full decode {case.pixel_counts[1]}")
    lines.append(f"the ROI bytes of both variants are equal in every round: {equal}")
    lines.append("")
    lines.append(f"{'selected':<10}{'variant':<9}{'reps':>6}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'spread ms':>11}   rounds (ms, host clock)")
    for (n, k), v in ms.items():
        lines.append(f"{n:<10}{k:<9}{reps[n, k]:>6}{med[n, k]:>11.3f}{min(v):>9.3f}{max(v):>9.3f}{spread[n, k]:>11.3f}   " + " ".join(f"{x:.3f}" for x in v))
    lines.append("")
    for n in cases:
        worst = max(s for (m, _), s in spread.items() if m == n)
        diff = med[n, "roi"] - med[n, "full"]
        verdict = "SLOWER than the full decode by more than the spread" if diff > worst else \
                  ("FASTER than the full decode by more than the spread" if -diff > worst else "within the spread of the full decode")
        lines.append(f"{n} selected: roi / full = {med[n, 'roi'] / med[n, 'full']:.2f} ({med[n, 'roi']:.3f} ms against {med[n, 'full']:.3f} ms), "
                     f"largest round-to-round spread {worst:.3f} ms: the ROI path is {verdict}")
    lines += trace_lines(a.kernel_trace, a.calls)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0 if equal else 2          # the times are a measurement, printed above; only unequal outputs are an error


if __name__ == "__main__":
    sys.exit(main())
