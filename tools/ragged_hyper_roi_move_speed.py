#!/usr/bin/env python3
"""What a MOVE of a 256 x 256 rectangle costs on a device-resident ragged HYPERPRIOR archive
(profiles/ragged_hyper_roi_move_speed.txt): hyperprior.MovingHyperpriorRoi against the only way before it, and against that way's
lower bound.

The workload of tools/ragged_hyper_roi_speed.py: the seeded mix of 64 image sizes, PARAM weights for the main transform, ONE archive
(sections z and y) of all of them, already in device memory, and the selections {3, 17, 40, 63} and {17}; once with y streams of
16384 symbols and once of 1024.  A 256 x 256 rectangle (clipped to the image) walks over seeded positions per image.  Per move,
timed with the host's clock and a synchronise per move:
  build   the only way before: codec.roi(rects) made for the position (window decoder, two cuts, window net), decode(archive=), dropped
  made    its lower bound: the RaggedHyperpriorRoi objects made before timing, decode(archive=) only
  move    MovingHyperpriorRoi made once and PREPARED once outside the timing (unpack, z coder, h_s, crop, parse, tables, scan); the
          position is written into the device tensor (a 16-byte device-to-device copy), decode(xy).  prepare's own time is
          reported beside it.
In every round the ROI bytes of the three must be equal at every position.

Method: all are warmed up; then they ALTERNATE in one process (one library serves all three) for --rounds rounds of the positions
each.  There is no ratio to meet: the table records the per-move medians and the largest round-to-round spread (max - min of the
rounds' means), and states the differences against it.

  python tools/ragged_hyper_roi_move_speed.py                                 the table
  python tools/ragged_hyper_roi_move_speed.py --only move --select 4 --stream-symbols 1024 --calls 32
      MovingHyperpriorRoi.decode alone, for a profiler run of its own:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ragged_hyper_roi_move_speed.py --only move ...
  python tools/ragged_hyper_roi_move_speed.py --kernel-trace 4@1024=PATH --calls 32 [--trace-only]
      adds the dispatch counts and device times of that run (SELECTED@SYMBOLS=path of the *_kernel_trace.csv)
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
STREAM_SYMBOLS = [16384, 1024]
SIDE = 256
POSITIONS = 16


def kernels_from_trace(path, n_calls):
    """rocprofv3 kernel trace -> ({kernel: [device ns per dispatch]}, dispatches) of the LAST n_calls moves: a move begins at a
    dispatch of the placement; what lies in front of the first of them (set-up, prepare, the warm-up) is cut off."""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    calls = []
    if rows:
        col = {k.lower(): k for k in rows[0]}
        rows.sort(key=lambda r: int(r[col["start_timestamp"]]))
        for r in rows:
            full = r[col["kernel_name"]]
            m = re.search(r"\b(k_[a-z0-9_]+)(<[^>]*>)?", full)
            name = (m.group(1) + (m.group(2) or "")) if m else "(runtime) " + full[:48]
            if name.startswith("k_ctx_roi_place"):
                calls.append([])
            if calls:
                calls[-1].append((name, int(r[col["end_timestamp"]]) - int(r[col["start_timestamp"]])))
    calls = calls[-n_calls:]
    if len(calls) > 1:                                           # what follows the last move's pixel cut is the final check()
        last = calls[-1]
        cut = max((i for i, (k, _) in enumerate(last) if k.startswith("k_ragged_cut")), default=len(last) - 1)
        calls[-1] = last[:cut + 1]
    per = defaultdict(list)
    for call in calls:
        for name, ns in call:
            per[name].append(ns)
    return per, calls


def trace_lines(specs, n_calls):
    lines = []
    for spec in specs:
        what, _, path = spec.partition("=")
        lines.append("")
        lines.append(f"kernels of {n_calls} moves, images @ y stream symbols {what}, from a profiler run of its own with nothing else in it (rocprofv3 "
                     f"--kernel-trace --stats --output-format csv -- tools/ragged_hyper_roi_move_speed.py --only move ...):")
        per, calls = kernels_from_trace(path, n_calls)
        n = max(len(calls), 1)
        for kern, ns in per.items():
            lines.append(f"  {kern:<52}{len(ns):6d} dispatches = {len(ns) / n:.2f} per move, median {statistics.median(ns) / 1e3:.2f} us "
                         f"(min {min(ns) / 1e3:.2f}, max {max(ns) / 1e3:.2f}), {sum(ns) / n / 1e3:.2f} us per move")
        total = sum(len(v) for v in per.values())
        lines.append(f"  {'all':<52}{total:6d} dispatches in {len(calls)} moves, {sorted({len(c) for c in calls})} per move (a move's own enqueued operations — 13 kernels "
                     f"with GDN and the band's memset, 14 — and, listed behind them, the 16-byte copy of the NEXT move's position), {sum(sum(v) for v in per.values()) / n / 1e3:.2f} us of device time per move")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["move"])
    ap.add_argument("--select", type=int, choices=sorted(SELECTIONS), default=4, help="with --only: the selection's size")
    ap.add_argument("--stream-symbols", type=int, choices=STREAM_SYMBOLS, default=1024, help="with --only: the y stream length")
    ap.add_argument("--calls", type=int, default=32)
    ap.add_argument("--kernel-trace", action="append", default=[], metavar="SELECTED@SYMBOLS=PATH")
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

    from simple_image_compression_network_amd import api, hyperprior

    sizes = make_sizes(a.seed, a.images)
    rng = np.random.default_rng(a.seed + 1)
    images = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in sizes]
    params = api.load_param_weights()

    def archive_of(wss):
        whole = hyperprior.RaggedHyperpriorCodec(sizes, seed=a.seed, main_params=params, y_stream_symbols=wss)
        whole.encode(whole.main.pack(images))
        b = whole.archive()
        torch.cuda.synchronize()
        return b, torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()

    class Case:
        """One selection of one archive: its codec, the positions, and the three variants."""

        def __init__(self, b, resident, sel, only_move=False):
            self.sel, self.resident = sel, resident
            self.codec = hyperprior.RaggedHyperpriorCodec.from_archive(b, seed=a.seed, main_params=params, images=sel)
            self.index = torch.tensor(sel, dtype=torch.int32, device="cuda")
            self.side = [(min(SIDE, w), min(SIDE, h)) for w, h in self.codec.sizes]
            prng = np.random.default_rng(a.seed + 2 + len(sel))
            self.positions = [[(int(prng.integers(0, w - rw + 1)), int(prng.integers(0, h - rh + 1))) for (w, h), (rw, rh) in
                               zip(self.codec.sizes, self.side)] for _ in range(POSITIONS)]
            self.rects = [[(x, y, rw, rh) for (x, y), (rw, rh) in zip(p, self.side)] for p in self.positions]
            self.made = [] if only_move else [self.codec.roi(r, **roi_direct.keywords(a)) for r in self.rects]
            self.moving = self.codec.moving_roi([(i, rw, rh) for i, (rw, rh) in enumerate(self.side)], **roi_direct.keywords(a))
            self.xy_all = torch.tensor(self.positions, dtype=torch.int32, device="cuda")
            self.xy = torch.zeros((len(sel), 2), dtype=torch.int32, device="cuda")
            self.pixels = torch.empty(self.moving.roi_bytes, dtype=torch.uint8, device="cuda")
            self.variants = {"build": self.by_build, "made": self.by_made, "move": self.by_move}
            self.streams = (self.moving.items, [tuple(int(v) for v in s.max_streams) for s in self.moving.layout],
                            [m.window.selected_streams for m in self.made])
            self.prepare()

        def prepare(self):
            self.moving.prepare(archive=self.resident, images=self.index)
            torch.cuda.synchronize()

        def by_build(self, k):
            roi = self.codec.roi(self.rects[k], **roi_direct.keywords(a))
            got = roi.decode(archive=self.resident, images=self.index, out=self.pixels)
            torch.cuda.synchronize()
            del roi
            return got

        def by_made(self, k):
            got = self.made[k].decode(archive=self.resident, images=self.index, out=self.pixels)
            torch.cuda.synchronize()
            return got

        def by_move(self, k):
            self.xy.copy_(self.xy_all[k])
            got = self.moving.decode(self.xy, out=self.pixels)
            torch.cuda.synchronize()
            return got

        def verify(self):
            ok = True
            for k in range(POSITIONS):
                want = self.by_made(k).reshape(-1).clone()
                self.made[k].check()
                self.pixels.zero_()
                ok &= bool(torch.equal(self.by_build(k).reshape(-1), want))
                self.pixels.zero_()
                ok &= bool(torch.equal(self.by_move(k).reshape(-1), want))      # (the others ran the front half again: same bytes in codec.s)
                ok &= not bool(self.moving.status[:, 0].any()) and not bool(self.moving.flags.any())
            return ok

    if a.only:
        b, resident = archive_of(a.stream_symbols)
        case = Case(b, resident, SELECTIONS[a.select], only_move=True)
        case.by_move(0)                                            # warm-up
        for k in range(a.calls):
            case.by_move(k % POSITIONS)
        case.moving.check()
        turn = iter(range(10 ** 9))

        def move():                                             # the positions in turn; the last call of a batch is position calls - 1
            case.xy.copy_(case.xy_all[next(turn) % a.calls % POSITIONS])
            return case.moving.decode(case.xy, out=case.pixels)
        roi_direct.timed_only(a, "ragged_hyper_roi_move", move, case.moving.views)
        print(f"{a.only}: {a.calls} moves done, {len(case.sel)} of {len(sizes)} images, y streams of {a.stream_symbols}")
        return 0

    cases, blobs = {}, {}
    for wss in STREAM_SYMBOLS:
        b, resident = archive_of(wss)
        blobs[wss] = len(b)
        for n, sel in SELECTIONS.items():
            cases[wss, n] = Case(b, resident, sel)
            print(f"made: {wss} symbols, {n} selected", file=sys.stderr, flush=True)
    equal = True
    for case in cases.values():
        equal &= case.verify()                                     # also the warm-up: every variant at every position

    def timed(fn):
        per = []
        for k in range(POSITIONS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(k)
            per.append((time.perf_counter() - t0) * 1e3)
        return per

    ms = {(c, k): [] for c, case in cases.items() for k in case.variants}
    prep = {c: [] for c in cases}
    for _ in range(a.rounds):
        for (c, k) in ms:
            if k == "move":                                        # the others left their own front half behind: prepare again, timed apart
                for _ in range(4):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    cases[c].prepare()
                    prep[c].append((time.perf_counter() - t0) * 1e3)
            ms[c, k].append(timed(cases[c].variants[k]))
        for case in cases.values():
            equal &= case.verify()
        print(f"round done, equal so far: {equal}", file=sys.stderr, flush=True)

    med = {k: statistics.median([x for r in v for x in r]) for k, v in ms.items()}
    means = {k: [statistics.mean(r) for r in v] for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in means.items()}
    lines = []
    lines.append(f"tools/ragged_hyper_roi_move_speed.py --seed {a.seed} --images {a.images} --rounds {a.rounds}")
    lines.append(f"device: {torch.cuda.get_device_name(0)}; hyperprior archives of {len(sizes)} images ({', '.join(f'{v} bytes at {k}' for k, v in blobs.items())} "
                 f"symbols per y stream), resident in device memory; a {SIDE} x {SIDE} rectangle, clipped to the image, at {POSITIONS} seeded positions per image")
    for (wss, n), case in cases.items():
        lines.append(f"{wss:>5} / {n} selected: images {case.sel}, sizes {case.codec.sizes}, rectangle sizes {case.side}")
        lines.append(f"   work items of the moving decode per set (its fixed capacity) {case.streams[0]}, stream capacities per slot {case.streams[1]}; "
                     f"streams a RaggedHyperpriorRoi made for the position selects: {min(case.streams[2])} .. {max(case.streams[2])}, "
                     f"mean {statistics.mean(case.streams[2]):.1f}")
    lines.append(f"the ROI bytes of the three variants are equal at every position in every round: {equal}")
    lines.append("")
    lines.append(f"{'symbols':<9}{'selected':<10}{'variant':<9}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'spread ms':>11}   round means (ms per move, host "
                 f"clock, a synchronise per move)")
    for ((wss, n), k), v in ms.items():
        flat = [x for r in v for x in r]
        lines.append(f"{wss:<9}{n:<10}{k:<9}{med[(wss, n), k]:>11.3f}{min(flat):>9.3f}{max(flat):>9.3f}{spread[(wss, n), k]:>11.3f}   " +
                     " ".join(f"{x:.3f}" for x in means[(wss, n), k]))
    lines.append("")
    for c in cases:
        worst = max(s for (m, _), s in spread.items() if m == c)
        below, under = med[c, "build"] - med[c, "move"], med[c, "made"] - med[c, "move"]
        lines.append(f"{c[0]} / {c[1]} selected: largest round-to-round spread {worst:.3f} ms; prepare (once per archive, outside the moves) "
                     f"median {statistics.median(prep[c]):.3f} ms (min {min(prep[c]):.3f}, max {max(prep[c]):.3f}, {len(prep[c])} calls)")
        lines.append(f"   build - move = {below:.3f} ms ({med[c, 'build']:.3f} against {med[c, 'move']:.3f}, {med[c, 'build'] / med[c, 'move']:.1f} x): move is "
                     f"{'below build by MORE than the spread' if below > worst else 'NOT below build by more than the spread'}")
        lines.append(f"   made - move  = {under:.3f} ms ({med[c, 'made']:.3f} against {med[c, 'move']:.3f}): move is "
                     f"{'BELOW made' if under > 0 else 'NOT below made: the expectation FAILS here (the surplus of the fixed capacity and the larger band cost more than the stages moved into prepare)'}"
                     f"{' by more than the spread' if under > worst else ('' if under <= 0 else '; the difference is within the spread')}")
    lines += trace_lines(a.kernel_trace, a.calls)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0 if equal else 2          # the times are a measurement, printed above; only unequal outputs are an error


if __name__ == "__main__":
    sys.exit(main())
