#!/usr/bin/env python3
"""What a MOVE of a 256 x 256 rectangle costs on a device-resident ragged archive (profiles/ragged_roi_move_speed.txt): the
moving ROI decode of library 0.17 against the only way before it, and against that way's lower bound.

The workload of tools/ragged_roi_speed.py: the seeded mix of 64 image sizes, PARAM weights, one archive of all of them, already in
device memory, unpacked ONCE into a coder's slots for the selections {3, 17, 40, 63} and {17}.  A 256 x 256 rectangle (clipped to
the image) walks over 32 seeded positions per image.  Per move, timed with the host's clock and a synchronise per move:
  build   the parent's only way: api.RaggedRoi made for the position (window decoder, two cuts, window net), decode, dropped
  made    its lower bound: the 32 RaggedRoi objects made before timing, decode only
  move    api.MovingRoi made once; the position is written into the device tensor (a 16-byte device-to-device copy), decode
In every round the ROI bytes of the three must be equal at every position.

Method: all are warmed up; then they ALTERNATE in one process (one library serves all three) for --rounds rounds of the 32
positions each.  There is no ratio to meet: the table records the per-move medians and the largest round-to-round spread
(max - min of the rounds' means), states both differences against it, and says plainly whether `move` is below `build` by more than
the spread and above `made`.

  python tools/ragged_roi_move_speed.py                                 the table
  python tools/ragged_roi_move_speed.py --only move --select 4 --calls 32
      MovingRoi.decode alone, for a profiler run of its own:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ragged_roi_move_speed.py --only move ...
  python tools/ragged_roi_move_speed.py --kernel-trace 4=PATH --calls 32 [--trace-only]
      adds the launch counts and device times of that run (SELECTED=path of the *_kernel_trace.csv)
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
POSITIONS = 32


def kernels_from_trace(path):
    """rocprofv3 kernel trace -> {kernel: [device ns per dispatch]} of the timed calls: everything from the first placement on."""
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
            continue                                            # not a kernel of this library
        started = started or "k_roi_place" in full
        if started:
            calls[m.group(1) + (m.group(2) or "")].append(int(r[col["end_timestamp"]]) - int(r[col["start_timestamp"]]))
    return calls


def trace_lines(specs, n_calls):
    lines = []
    for spec in specs:
        selected, _, path = spec.partition("=")
        lines.append("")
        lines.append(f"kernels of {n_calls} moves, {selected} image(s), from a profiler run of its own (rocprofv3 --kernel-trace --stats "
                     f"--output-format csv -- tools/ragged_roi_move_speed.py --only move --select {selected} --calls {n_calls}):")
        calls = kernels_from_trace(path)
        for kern, ns in sorted(calls.items()):
            lines.append(f"  {kern:<44}{len(ns):6d} dispatches = {len(ns) / n_calls:.2f} per move, median {statistics.median(ns) / 1e3:.2f} us "
                         f"(min {min(ns) / 1e3:.2f}, max {max(ns) / 1e3:.2f})")
        total = sum(len(v) for v in calls.values())
        lines.append(f"  {'all':<44}{total:6d} dispatches = {total / n_calls:.2f} per move (9 expected), "
                     f"{sum(sum(v) for v in calls.values()) / n_calls / 1e3:.2f} us of device time per move")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["move"])
    ap.add_argument("--select", type=int, choices=sorted(SELECTIONS), default=4, help="with --only: the selection's size")
    ap.add_argument("--calls", type=int, default=POSITIONS)
    ap.add_argument("--kernel-trace", action="append", default=[], metavar="SELECTED=PATH")
    ap.add_argument("--trace-only", action="store_true", help="print the --kernel-trace sections alone (no device needed)")
    ap.add_argument("--out", help="also write the table to this file")
    roi_direct.add_arguments(ap)
    a = ap.parse_args()
    roi_direct.check(ap, a)
    if a.rounds < 3 and not a.only:
        ap.error("--rounds: at least 3")
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
        """One selection: its net and coder with the archive unpacked into it once, the positions, and the three variants."""

        def __init__(self, sel):
            self.sel = sel
            self.net = api.RaggedNet.from_archive(b, images=sel, shared_weights=weights)
            self.coder = self.net.latent_coder([lengths[i] for i in sel])
            self.archive = codec.RaggedArchive([self.coder], tag=0)
            self.valid, = self.archive.unpack(resident, images=torch.tensor(sel, dtype=torch.int32, device="cuda"))
            self.archive.check()
            self.side = [(min(SIDE, w), min(SIDE, h)) for w, h in self.net.sizes]
            prng = np.random.default_rng(a.seed + 2 + len(sel))
            self.positions = [[(int(prng.integers(0, w - rw + 1)), int(prng.integers(0, h - rh + 1))) for (w, h), (rw, rh) in
                               zip(self.net.sizes, self.side)] for _ in range(POSITIONS)]
            self.rects = [[(x, y, rw, rh) for (x, y), (rw, rh) in zip(p, self.side)] for p in self.positions]
            self.made = [] if a.only else [api.RaggedRoi(self.net, r, coder=self.coder, **roi_direct.keywords(a)) for r in self.rects]
            self.moving = self.net.moving_roi([(i, rw, rh) for i, (rw, rh) in enumerate(self.side)], coder=self.coder,
                                              **roi_direct.keywords(a))
            self.xy_all = torch.tensor(self.positions, dtype=torch.int32, device="cuda")
            self.xy = torch.zeros((len(sel), 2), dtype=torch.int32, device="cuda")
            self.pixels = torch.empty(self.moving.roi_bytes, dtype=torch.uint8, device="cuda")
            self.variants = {"build": self.by_build, "made": self.by_made, "move": self.by_move}
            self.streams = (self.moving.items, [m.window.selected_streams for m in self.made])

        def by_build(self, k):
            roi = api.RaggedRoi(self.net, self.rects[k], coder=self.coder, **roi_direct.keywords(a))
            got = roi.decode(valid=self.valid, out=self.pixels)
            torch.cuda.synchronize()
            del roi
            return got

        def by_made(self, k):
            got = self.made[k].decode(valid=self.valid, out=self.pixels)
            torch.cuda.synchronize()
            return got

        def by_move(self, k):
            self.xy.copy_(self.xy_all[k])
            got = self.moving.decode(self.xy, valid=self.valid, out=self.pixels)
            torch.cuda.synchronize()
            return got

        def verify(self):
            ok = True
            for k in range(POSITIONS):
                want = self.by_made(k).reshape(-1).clone()
                self.pixels.zero_()
                ok &= bool(torch.equal(self.by_move(k).reshape(-1), want))
                self.pixels.zero_()
                ok &= bool(torch.equal(self.by_build(k).reshape(-1), want))
                ok &= not bool(self.moving.status[:, 0].any()) and not bool(self.moving.flags.any())
            return ok

    if a.only:
        case = Case(SELECTIONS[a.select])
        torch.cuda.synchronize()
        for k in range(a.calls):
            case.by_move(k % POSITIONS)
        assert not case.moving.status[:, 0].any()
        turn = iter(range(10 ** 9))

        def move():                                             # the positions in turn; the last call of a batch is position calls - 1
            case.xy.copy_(case.xy_all[next(turn) % a.calls % POSITIONS])
            return case.moving.decode(case.xy, valid=case.valid, out=case.pixels)
        roi_direct.timed_only(a, "ragged_roi_move", move, case.moving.views)
        print(f"{a.only}: {a.calls} moves done, {len(case.sel)} of {len(sizes)} images")
        return 0

    cases = {n: Case(sel) for n, sel in SELECTIONS.items()}
    equal = True
    for case in cases.values():
        equal &= case.verify()                                 # also the warm-up: every variant at every position

    def timed(fn):
        per = []
        for k in range(POSITIONS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(k)
            per.append((time.perf_counter() - t0) * 1e3)
        return per

    ms = {(n, k): [] for n, case in cases.items() for k in case.variants}
    for _ in range(a.rounds):
        for (n, k) in ms:
            ms[n, k].append(timed(cases[n].variants[k]))
        for case in cases.values():
            equal &= case.verify()

    med = {k: statistics.median([x for r in v for x in r]) for k, v in ms.items()}
    means = {k: [statistics.mean(r) for r in v] for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in means.items()}
    lines = []
    lines.append(f"tools/ragged_roi_move_speed.py --seed {a.seed} --images {a.images} --rounds {a.rounds}")
    lines.append(f"device: {torch.cuda.get_device_name(0)}; an archive of {len(sizes)} images, {len(b)} bytes, resident in device memory and "
                 f"unpacked once per selection; a {SIDE} x {SIDE} rectangle, clipped to the image, at {POSITIONS} seeded positions per image")
    for n, case in cases.items():
        lines.append(f"{n} selected: images {case.sel}, sizes {case.net.sizes}, rectangle sizes {case.side}")
        lines.append(f"   work items of the moving decode (its fixed capacity) {case.streams[0]}; streams a RaggedRoi made for the position "
                     f"selects: {min(case.streams[1])} .. {max(case.streams[1])}, mean {statistics.mean(case.streams[1]):.1f}")
    lines.append(f"the ROI bytes of the three variants are equal at every position in every round: {equal}")
    lines.append("")
    lines.append(f"{'selected':<10}{'variant':<9}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'spread ms':>11}   round means (ms per move, host clock, "
                 f"a synchronise per move)")
    for (n, k), v in ms.items():
        flat = [x for r in v for x in r]
        lines.append(f"{n:<10}{k:<9}{med[n, k]:>11.3f}{min(flat):>9.3f}{max(flat):>9.3f}{spread[n, k]:>11.3f}   " + " ".join(f"{x:.3f}" for x in means[n, k]))
    lines.append("")
    for n in cases:
        worst = max(s for (m, _), s in spread.items() if m == n)
        below, above = med[n, "build"] - med[n, "move"], med[n, "move"] - med[n, "made"]
        lines.append(f"{n} selected: largest round-to-round spread {worst:.3f} ms")
        lines.append(f"   build - move = {below:.3f} ms ({med[n, 'build']:.3f} against {med[n, 'move']:.3f}, {med[n, 'build'] / med[n, 'move']:.1f} x): "
                     f"move is {'below build by MORE than the spread' if below > worst else 'NOT below build by more than the spread: the expectation FAILS'}")
        lines.append(f"   move - made  = {above:.3f} ms ({med[n, 'move']:.3f} against {med[n, 'made']:.3f}): move is "
                     f"{'above made, as expected (the placement launch and the streams the fixed capacity adds)' if above > 0 else 'NOT above made: the expectation FAILS (it is at or below the lower bound)'}"
                     f"{'' if abs(above) > worst else '; the difference is within the spread'}")
    lines += trace_lines(a.kernel_trace, a.calls)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0 if equal else 2          # the times are a measurement, printed above; only unequal outputs are an error


if __name__ == "__main__":
    sys.exit(main())
