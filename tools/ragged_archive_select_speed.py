#!/usr/bin/env python3
"""A few images out of a ragged archive: the routes from an archive of 64 to the reconstructions of 4 of them and of 1
(profiles/ragged_archive_select_speed.txt).

The workload of tools/ragged_archive_speed.py: the seeded mix of 64 image sizes, PARAM weights, one archive of all of them
(RaggedNet.compress_archive, before timing).  For a selection `sel`, with the net for those images made before timing
(RaggedNet.from_archive(b, images=sel)):
  (a) split     codec.split_archive(b) on the host, then net.decompress([containers of sel]): the only way before library 0.11 —
                RaggedLatentCoder.for_containers (a new coder object, a zeroed host buffer of the slots' full capacity, one copy per
                container, one upload), decode, layers 4-7
  (b) select    net.decompress_archive(b, images=sel): the headers read on the host, the WHOLE archive uploaded, the two launches of
                sicn_ragged_archive_unpack_select_async, decode, layers 4-7
  (c) subset    codec.subset_archive(b, sel) on the host, then net.decompress_archive(small): only the selection is uploaded
  (d) resident  the archive already lies in device memory and the index array too: unpack(images=) + decode + layers 4-7 on
                objects made before timing — (b) without its upload and without its host-side reading of the headers
Every variant ends with the device idle and is timed with the host's clock (what differs between them is host work and PCIe).

Method: every variant is warmed up; then the variants ALTERNATE in one process for --rounds rounds, each timed around enough
back-to-back repetitions to fill --seconds.  In every round every variant's reconstructions must be, byte for byte, the selected
images' rows of the full decompress_archive(b).  There is no ratio to meet: the table records the times and the largest
round-to-round spread (max - min over the rounds).

  python tools/ragged_archive_select_speed.py                                   the table
  python tools/ragged_archive_select_speed.py --only select --select 1 --calls 20        variant (d)'s unpack alone, for a profiler run of its own:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ragged_archive_select_speed.py --only select --select 1 --calls 20
  python tools/ragged_archive_select_speed.py --kernel-trace 1=DIR/.../*_kernel_trace.csv --kernel-trace 4=... --calls 20
      adds the launch counts and device times of those runs (SELECTED=PATH); with --trace-only, prints those sections alone
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

from ragged_speed import make_sizes  # noqa: E402  (the same seeded mix)

SELECTIONS = {4: [3, 17, 40, 63], 1: [17]}


def kernels_from_trace(path):
    """rocprofv3 kernel trace -> ({kernel of the select-unpacks: [device ns per dispatch]}, {kernel of the set-up: count}).  The
    archive kernels in start order: a copy belongs to the parser in front of it, and the `--only select` run packs the archive and
    unpacks it whole once (index + copy<pack>, parse + copy<unpack>) before its calls."""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    calls, setup = defaultdict(list), defaultdict(int)
    if not rows:
        return calls, setup
    col = {k.lower(): k for k in rows[0]}
    rows.sort(key=lambda r: int(r[col["start_timestamp"]]))
    before = None
    for r in rows:
        m = re.search(r"\bk_archive_(index|parse_select|parse|copy)\b", r[col["kernel_name"]])
        if not m:
            continue
        name = m.group(0)
        if name == "k_archive_copy":
            name += "<pack>" if re.search(r"copy<\(?(bool\))?(true|1)", r[col["kernel_name"]]) else "<unpack>"
        if name == "k_archive_parse_select" or (name == "k_archive_copy<unpack>" and before == "k_archive_parse_select"):
            calls[name].append(int(r[col["end_timestamp"]]) - int(r[col["start_timestamp"]]))
        else:
            setup[name] += 1
        before = name
    return calls, setup


def trace_lines(specs, n_calls):
    lines = []
    for spec in specs:
        selected, _, path = spec.partition("=")
        lines.append("")
        lines.append(f"kernels, from a profiler run of its own (rocprofv3 --kernel-trace --stats --output-format csv -- "
                     f"tools/ragged_archive_select_speed.py --only select --select {selected} --calls {n_calls}):")
        calls, setup = kernels_from_trace(path)
        for kern, ns in sorted(calls.items()):
            lines.append(f"  {kern:<24}{len(ns):6d} dispatches = {len(ns) / n_calls:.2f} per call, median {statistics.median(ns) / 1e3:.2f} us "
                         f"(min {min(ns) / 1e3:.2f}, max {max(ns) / 1e3:.2f})")
        total = sum(len(v) for v in calls.values())
        lines.append(f"  {'all':<24}{total:6d} dispatches = {total / n_calls:.2f} per select-unpack (2 expected)")
        lines.append("  before the calls, making the archive and the reference: " + ", ".join(f"{v} {k}" for k, v in sorted(setup.items())))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--only", choices=["select"])
    ap.add_argument("--select", type=int, choices=sorted(SELECTIONS), default=4, help="with --only: the selection's size")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernel-trace", action="append", default=[], metavar="SELECTED=PATH",
                    help="a rocprofv3 *_kernel_trace.csv of an `--only select --select SELECTED --calls N` run: print its launches and device times")
    ap.add_argument("--trace-only", action="store_true", help="print the --kernel-trace sections alone (no device needed)")
    ap.add_argument("--out", help="also write the table to this file")
    a = ap.parse_args()
    if a.rounds < 5 and not a.only:
        ap.error("--rounds: at least 5")
    if a.trace_only:                                            # no device needed
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
    full = api.RaggedNet(sizes, shared_weights=weights)
    b = full.compress_archive(full.pack(images))
    want_all = [v.clone() for v in full.views(7, full.decompress_archive(b))]
    torch.cuda.synchronize()
    resident = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    lengths = [int(h[0].stream_symbols) for h in codec.archive_info(b)["headers"]]

    class Case:
        """One selection: its net, the objects variant (d) needs, the four variants; all made before timing."""

        def __init__(self, sel):
            self.sel = sel
            self.net = api.RaggedNet.from_archive(b, images=sel, shared_weights=weights)
            self.want = self.net.pack([want_all[i] for i in sel], layer=7)
            self.coder = self.net.latent_coder([lengths[i] for i in sel])
            self.archive = codec.RaggedArchive([self.coder], tag=0)
            self.index = torch.tensor(sel, dtype=torch.int32, device="cuda")
            self.latent = torch.empty(self.net.nbytes(3), dtype=torch.uint8, device="cuda")
            self.out = torch.empty(self.net.nbytes(7), dtype=torch.uint8, device="cuda")
            self.subset_bytes = len(codec.subset_archive(b, sel))
            self.variants = {"split": self.split, "select": self.select, "subset": self.subset, "resident": self.from_resident}

        def split(self):
            rows = codec.split_archive(b)
            out = self.net.decompress([rows[i][0] for i in self.sel], out=self.out)
            torch.cuda.synchronize()
            return out

        def select(self):
            out = self.net.decompress_archive(b, out=self.out, images=self.sel)
            torch.cuda.synchronize()
            return out

        def subset(self):
            out = self.net.decompress_archive(codec.subset_archive(b, self.sel), out=self.out)
            torch.cuda.synchronize()
            return out

        def unpack_resident(self):
            return self.archive.unpack(resident, images=self.index)

        def from_resident(self):
            valid, = self.unpack_resident()
            self.coder.decode(self.latent, valid=valid)
            out, _ = self.net.run_layers(4, 7, self.latent, out=self.out)
            torch.cuda.synchronize()
            return out

        def verify(self):
            ok = True
            for fn in self.variants.values():
                self.out.zero_()
                ok &= bool(torch.equal(fn(), self.want))
            self.archive.check()
            self.coder.check()
            return ok

    if a.only:
        case = Case(SELECTIONS[a.select])
        for _ in range(a.calls):
            case.unpack_resident()
        torch.cuda.synchronize()
        case.archive.check()
        print(f"select: {a.calls} calls of unpack(images=) done, {len(case.sel)} of {len(sizes)} images")
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
    lines.append(f"tools/ragged_archive_select_speed.py --seed {a.seed} --images {a.images} --rounds {a.rounds} --seconds {a.seconds}")
    lines.append(f"device: {torch.cuda.get_device_name(0)}; an archive of {len(sizes)} images, {len(b)} bytes; selections "
                 + "; ".join(f"{n}: images {case.sel}, {case.subset_bytes} bytes as an archive of their own, {case.coder.slot_bytes} bytes of slots"
                             for n, case in cases.items()))
    lines.append(f"every variant's reconstructions are the selected images' rows of the full decompress_archive, byte for byte, in every round: {equal}")
    lines.append("")
    lines.append(f"{'selected':<10}{'variant':<10}{'PCIe bytes':>12}{'reps':>6}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'spread ms':>11}   rounds (ms, host clock)")
    for (n, k), v in ms.items():
        case = cases[n]
        pcie = {"split": case.coder.slot_bytes + 8 * n, "select": len(b) + 4 * n, "subset": case.subset_bytes, "resident": 0}[k]
        lines.append(f"{n:<10}{k:<10}{pcie:>12}{reps[n, k]:>6}{med[n, k]:>11.3f}{min(v):>9.3f}{max(v):>9.3f}{spread[n, k]:>11.3f}   "
                     + " ".join(f"{x:.3f}" for x in v))
    lines.append("")
    for n in cases:
        worst = max(s for (m, _), s in spread.items() if m == n)
        lines.append(f"{n} selected: largest round-to-round spread of any variant {worst:.3f} ms; from host bytes select / subset = "
                     f"{med[n, 'select'] / med[n, 'subset']:.2f}, select / split = {med[n, 'select'] / med[n, 'split']:.2f}, "
                     f"subset / split = {med[n, 'subset'] / med[n, 'split']:.2f}; resident / select = {med[n, 'resident'] / med[n, 'select']:.2f}")
    lines += trace_lines(a.kernel_trace, a.calls)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0 if equal else 2          # the times are a measurement, printed above; only unequal outputs are an error


if __name__ == "__main__":
    sys.exit(main())
