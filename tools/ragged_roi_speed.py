#!/usr/bin/env python3
"""A 256 x 256 detail of a few images out of a device-resident ragged archive: the ROI path of library 0.12 against the only way
before it, the full decode of the same images and a slice (profiles/ragged_roi_speed.txt).

The workload of tools/ragged_archive_select_speed.py: the seeded mix of 64 image sizes, PARAM weights, one archive of all of them,
already in device memory, and the selections {3, 17, 40, 63} and {17}.  The rectangle is 256 x 256, centred, clipped to the image.
For a selection, on objects made before timing:
  full   RaggedArchive.unpack(images=) + RaggedLatentCoder.decode + layers 4-7 over the whole images, then the rectangle sliced
         out of every reconstruction (a view and one copy per image)
  roi    RaggedArchive.unpack(images=) + RaggedRoi.decode: the window decoder over the streams that hold the latent rows, the cut of
         the latent columns, layers 4-7 over the windows, the cut of the rectangle — 2 + 1 + 4 + 1 launches behind the unpack
Both end with the device idle and are timed with the host's clock.

Method: both variants are warmed up; then they ALTERNATE in one process for --rounds rounds, each timed around enough back-to-back
repetitions to fill --seconds.  In every round the ROI bytes of both must be equal.  There is no ratio to meet: the table records
the times and the largest round-to-round spread (max - min over the rounds), and says whether the ROI path was slower than the full
decode by more than that spread.

  python tools/ragged_roi_speed.py                                    the table
  python tools/ragged_roi_speed.py --only roi --select 4 --calls 20   RaggedRoi.decode alone (--only window: the window decoder alone),
      for a profiler run of its own:  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ragged_roi_speed.py --only roi ...
  python tools/ragged_roi_speed.py --kernel-trace roi:4=PATH --kernel-trace window:1=PATH ... --calls 20 [--trace-only]
      adds the launch counts and device times of those runs (WHAT:SELECTED=path of the *_kernel_trace.csv)
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


def centred(size):
    w, h = size
    rw, rh = min(SIDE, w), min(SIDE, h)
    return ((w - rw) // 2, (h - rh) // 2, rw, rh)


def kernels_from_trace(path):
    """rocprofv3 kernel trace -> {kernel: [device ns per dispatch]} of the timed calls: everything from the first dispatch of the
    window decoder on (an `--only` run launches nothing else of the library's after its set-up)."""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    calls = defaultdict(list)
    if not rows:
        return calls
    col = {k.lower(): k for k in rows[0]}
    rows.sort(key=lambda r: int(r[col["start_timestamp"]]))
    started = False
    for r in rows:
        full = r[col["kernel_name"]]
        m = re.search(r"\b(k_[a-z0-9_]+)(<[^>]*>)?", full)
        if not m:
            continue                                            # not a kernel of this library (the final check()'s read-back copies)
        name = m.group(1) + (m.group(2) or "")
        started = started or "k_ragged_decode_window" in full
        if started:
            calls[name].append(int(r[col["end_timestamp"]]) - int(r[col["start_timestamp"]]))
    return calls


def trace_lines(specs, n_calls):
    lines = []
    for spec in specs:
        what, _, path = spec.partition("=")
        kind, _, selected = what.partition(":")
        expected = {"roi": 8, "window": 2}.get(kind, 0)
        lines.append("")
        lines.append(f"kernels of {n_calls} calls, {selected} image(s), from a profiler run of its own (rocprofv3 --kernel-trace --stats "
                     f"--output-format csv -- tools/ragged_roi_speed.py --only {kind} --select {selected} --calls {n_calls}):")
        calls = kernels_from_trace(path)
        for kern, ns in sorted(calls.items()):
            lines.append(f"  {kern:<44}{len(ns):6d} dispatches = {len(ns) / n_calls:.2f} per call, median {statistics.median(ns) / 1e3:.2f} us "
                         f"(min {min(ns) / 1e3:.2f}, max {max(ns) / 1e3:.2f})")
        total = sum(len(v) for v in calls.values())
        lines.append(f"  {'all':<44}{total:6d} dispatches = {total / n_calls:.2f} per call ({expected} expected), "
                     f"{sum(sum(v) for v in calls.values()) / n_calls / 1e3:.2f} us of device time per call")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--only", choices=["roi", "window"])
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

    from simple_image_compression_network_amd import api, codec
    from simple_image_compression_network_amd.config import eight_layer_descs

    sizes = make_sizes(a.seed, a.images)
    rng = np.random.default_rng(a.seed + 1)
    images = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for w, h in sizes]
    weights = [api.DeviceWeights(d, w, b) for d, (w, b) in zip(eight_layer_descs(16, 16), api.load_param_weights())]
    whole = api.RaggedNet(sizes, shared_weights=weights)
    b = whole.compress_archive(whole.pack(images))
    torch.cuda.synchronize()
    resident = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    lengths = [int(h[0].stream_symbols) for h in codec.archive_info(b)["headers"]]
    del whole, images

    class Case:
        """One selection: its net, coder, archive object and RaggedRoi, all made before timing."""

        def __init__(self, sel):
            self.sel = sel
            self.net = api.RaggedNet.from_archive(b, images=sel, shared_weights=weights)
            self.rects = [centred(s) for s in self.net.sizes]
            self.coder = self.net.latent_coder([lengths[i] for i in sel])
            self.archive = codec.RaggedArchive([self.coder], tag=0)
            self.index = torch.tensor(sel, dtype=torch.int32, device="cuda")
            self.roi = api.RaggedRoi(self.net, self.rects, coder=self.coder, **roi_direct.keywords(a))
            self.latent = torch.empty(self.net.nbytes(3), dtype=torch.uint8, device="cuda")
            self.out = torch.empty(self.net.nbytes(7), dtype=torch.uint8, device="cuda")
            self.pixels = torch.empty(sum(3 * r[2] * r[3] for r in self.rects), dtype=torch.uint8, device="cuda")
            self.variants = {"full": self.full, "roi": self.by_roi}
            self.streams = (self.roi.window.selected_streams, sum(int(im.n_streams) for im in self.coder.images[:len(sel)]))
            self.latent_positions = (sum(p["cw"] * p["rh"] for p in self.roi.plans), sum(h * w for h, w, _ in self.net.shapes(3)))
            self.pixel_counts = (sum(256 * p["cw"] * p["rh"] for p in self.roi.plans), sum(h * w for h, w, _ in self.net.shapes(7)),
                                 sum(r[2] * r[3] for r in self.rects))

        def full(self):
            valid, = self.archive.unpack(resident, images=self.index)
            self.coder.decode(self.latent, valid=valid)
            out, _ = self.net.run_layers(4, 7, self.latent, out=self.out)
            got = torch.cat([v[y0:y0 + h, x0:x0 + w].reshape(-1) for v, (x0, y0, w, h) in zip(self.net.views(7, out), self.rects)])
            torch.cuda.synchronize()
            return got

        def by_roi(self):
            valid, = self.archive.unpack(resident, images=self.index)
            got = self.roi.decode(valid=valid, out=self.pixels)
            torch.cuda.synchronize()
            return got

        def verify(self):
            self.pixels.zero_()
            ok = bool(torch.equal(self.by_roi(), self.full()))
            self.archive.check()
            self.coder.check()
            self.roi.window.check()
            return ok

    if a.only:
        case = Case(SELECTIONS[a.select])
        valid, = case.archive.unpack(resident, images=case.index)
        torch.cuda.synchronize()
        band = torch.empty(case.roi.window.band_bytes, dtype=torch.uint8, device="cuda")
        if a.only == "roi":
            roi_direct.timed_only(a, "ragged_roi", lambda: case.roi.decode(valid=valid, out=case.pixels), case.roi.views)
        for _ in range(a.calls):
            if a.only == "roi":
                case.roi.decode(valid=valid, out=case.pixels)
            else:
                case.roi.window.decode(band, valid=valid)
        torch.cuda.synchronize()
        case.roi.window.check()
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
    lines.append(f"tools/ragged_roi_speed.py --seed {a.seed} --images {a.images} --rounds {a.rounds} --seconds {a.seconds}")
    lines.append(f"device: {torch.cuda.get_device_name(0)}; an archive of {len(sizes)} images, {len(b)} bytes, resident in device memory; "
                 f"a centred {SIDE} x {SIDE} rectangle, clipped to the image")
    for n, case in cases.items():
        lines.append(f"{n} selected: images {case.sel}, sizes {case.net.sizes}, rectangles {case.rects}")
        lines.append(f"   streams selected / total {case.streams[0]} / {case.streams[1]}; latent positions in the windows / in the images "
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
        verdict = "slower than the full decode by MORE than the spread" if med[n, "roi"] - med[n, "full"] > worst else \
                  ("no slower than the full decode beyond the spread" if med[n, "roi"] >= med[n, "full"] else "faster than the full decode")
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
