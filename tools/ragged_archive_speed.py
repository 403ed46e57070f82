#!/usr/bin/env python3
"""Ragged archive against the host loop it replaces: "encode -> bytes on the host" and back (profiles/ragged_archive_speed.txt).

The workload of tools/ragged_coder_speed.py: the seeded mix of 64 image sizes, PARAM weights, its boundary-3 latents (one RaggedNet
call, before timing) through one codec.RaggedLatentCoder.  To the host:
  containers   coder.encode, then coder.containers(): synchronise, copy the WHOLE slot buffer (every slot at the capacity of an
               incompressible latent) to the host, slice it in Python — what the library did before 0.10
  archive      coder.encode, RaggedArchive.pack (2 launches), read the 16-byte status, copy exactly status.bytes into a pinned host
               buffer
and back:
  containers   RaggedLatentCoder.for_containers (a new coder object, a zeroed host buffer of full capacity, n copies, one upload),
               then decode
  refill       the same host loop into an EXISTING coder's buffers (no object is created), then decode
  archive      upload of the archive from the pinned buffer, RaggedArchive.unpack (2 launches), decode with the valid array it gives
Every variant ends with the device idle, and is timed with the host's clock (the work being measured is host work and PCIe).

Method: every variant is warmed up; then the variants ALTERNATE in one process for --rounds rounds, each timed around enough
back-to-back repetitions to fill --seconds.  In every round the archive must split to `containers`' containers and the decoded latents
must be the encoder's input.  Verdict, per direction: archive's median must be below containers' median by more than the largest
round-to-round spread (max - min over the rounds) of any variant of that direction.

  python tools/ragged_archive_speed.py                              the table
  python tools/ragged_archive_speed.py --only archive --calls 20 [--images 1]     pack + unpack only, for a profiler run of its own:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ragged_archive_speed.py --only archive --calls 20
  python tools/ragged_archive_speed.py --kernel-trace 64=DIR/.../*_kernel_trace.csv [--kernel-trace 1=...] --calls 20
      adds the launch counts and device times of those runs (IMAGES=PATH; the copy kernels' rate for the run whose IMAGES is --images)
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


def kernels_from_trace(path):
    """rocprofv3 kernel trace -> {archive kernel name: [device ns per dispatch]} (pack and unpack forms of the copy kept apart)."""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    out = defaultdict(list)
    if not rows:
        return out
    col = {k.lower(): k for k in rows[0]}
    for r in rows:
        m = re.search(r"\bk_archive_(index|parse|copy)\b(<[^>]*>)?", r[col["kernel_name"]])
        if m:
            name = m.group(0) if m.group(1) != "copy" else "k_archive_copy" + ("<pack>" if re.search(r"copy<\(?(bool\))?(true|1)", m.group(0)) else "<unpack>")
            out[name].append(int(r[col["end_timestamp"]]) - int(r[col["start_timestamp"]]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--only", choices=["archive"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernel-trace", action="append", default=[], metavar="IMAGES=PATH",
                    help="a rocprofv3 *_kernel_trace.csv of an `--only archive --calls N --images IMAGES` run: print its launches and device times")
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
    lat, _ = net.run_layers(0, 3, net.pack(images))
    torch.cuda.synchronize()
    symbols = lat.numel()

    # ---- every buffer is allocated before timing
    coder = net.latent_coder()
    archive = codec.RaggedArchive([coder], tag=0)
    archive.buffer = torch.empty(archive.max_bytes, dtype=torch.uint8, device="cuda")     # pack()'s buffer, made here: no launch before the calls
    pinned = torch.empty(archive.max_bytes, dtype=torch.uint8).pin_memory()
    status_host = torch.empty(4, dtype=torch.int32).pin_memory()
    dec = net.latent_coder()                                    # the decoder side: its own slots
    dec_archive = codec.RaggedArchive([dec], tag=0)
    dev_in = torch.empty(archive.max_bytes, dtype=torch.uint8, device="cuda")
    back = torch.empty_like(lat)
    n = len(sizes)
    state = {}

    def enc_containers():
        coder.encode(lat)
        state["containers"] = coder.containers()

    def enc_archive():
        coder.encode(lat)
        archive.pack()
        status_host.copy_(archive.status)                       # synchronises: 16 bytes
        nbytes = (int(status_host[2]) & 0xFFFFFFFF) | (int(status_host[3]) & 0xFFFFFFFF) << 32
        if int(status_host[0]):
            raise RuntimeError(f"pack status {int(status_host[0]):#x}")
        pinned[:nbytes].copy_(archive.buffer[:nbytes])          # exactly the archive
        torch.cuda.synchronize()
        state["nbytes"] = nbytes

    def dec_containers():
        other = codec.RaggedLatentCoder.for_containers(state["containers"])
        other.decode(back)
        torch.cuda.synchronize()
        state["other"] = other

    def dec_refill():
        host = torch.zeros(dec.slot_bytes, dtype=torch.uint8)
        for c, im in zip(state["containers"], dec.images):
            host[int(im.slot_offset):int(im.slot_offset) + len(c)] = torch.frombuffer(bytearray(c), dtype=torch.uint8)
        dec.slot_buffer.copy_(host)
        dec.enc_status.copy_(torch.tensor([[0, len(c)] for c in state["containers"]], dtype=torch.int32))
        dec.decode(back)
        torch.cuda.synchronize()

    def dec_archive_fn():
        nbytes = state["nbytes"]
        dev_in[:nbytes].copy_(pinned[:nbytes], non_blocking=True)
        valid, = dec_archive.unpack(dev_in[:nbytes])
        dec.decode(back, valid=valid)
        torch.cuda.synchronize()

    if a.only:
        for _ in range(a.calls):
            coder.encode(lat)
            archive.pack()
            valid, = dec_archive.unpack(archive.buffer)
            dec.decode(back, valid=valid)
        torch.cuda.synchronize()
        archive.check()
        dec_archive.check()
        print(f"archive: {a.calls} calls of encode + pack + unpack + decode done, {n} images")
        return 0

    to_host = {"containers": enc_containers, "archive": enc_archive}
    to_device = {"containers": dec_containers, "refill": dec_refill, "archive": dec_archive_fn}

    def verify():
        ok = codec.split_archive(pinned[:state["nbytes"]].numpy().tobytes()) == [(c,) for c in state["containers"]]
        for fn in to_device.values():
            back.zero_()
            fn()
            ok &= torch.equal(back, lat)
        dec.check()
        dec_archive.check()
        state["other"].check()
        return ok

    for fn in list(to_host.values()) * 2:
        fn()
    equal = verify()

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    ms, reps = {}, {}
    for group, variants in (("to host", to_host), ("to device", to_device)):
        for k, fn in variants.items():
            reps[group, k] = max(2, int(a.seconds * 1e3 / timed(fn, 3)) + 1)
            ms[group, k] = []
    for _ in range(a.rounds):
        for (group, k) in ms:
            ms[group, k].append(timed(to_host[k] if group == "to host" else to_device[k], reps[group, k]))
        equal &= verify()

    coded = sum(len(c) for c in state["containers"])
    nbytes = state["nbytes"]
    pcie = {("to host", "containers"): coder.slot_bytes + 8 * n, ("to host", "archive"): nbytes + 16,
            ("to device", "containers"): coder.slot_bytes + 8 * n, ("to device", "refill"): coder.slot_bytes + 8 * n,
            ("to device", "archive"): nbytes}
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}

    lines = []
    lines.append(f"tools/ragged_archive_speed.py --seed {a.seed} --images {a.images} --rounds {a.rounds} --seconds {a.seconds}")
    lines.append(f"device: {torch.cuda.get_device_name(0)}; {n} latents, {symbols / 1e6:.2f} M symbols; {coded / 1e6:.2f} MB of containers "
                 f"({8 * coded / symbols:.2f} bit / symbol) in {coder.slot_bytes / 1e6:.2f} MB of slots; archive {nbytes} bytes "
                 f"(+{nbytes - coded} for header, index and alignment); chunk {int(api._lib.lib().sicn_ragged_archive_chunk_bytes())} bytes")
    lines.append(f"archive splits to containers()' containers and every variant decodes to the encoder's input, in every round: {equal}")
    lines.append("")
    lines.append(f"{'direction':<11}{'variant':<12}{'PCIe bytes':>12}{'reps':>6}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'spread ms':>11}   rounds (ms, host clock)")
    for (group, k), v in ms.items():
        lines.append(f"{group:<11}{k:<12}{pcie[group, k]:>12}{reps[group, k]:>6}{med[group, k]:>11.3f}{min(v):>9.3f}{max(v):>9.3f}{spread[group, k]:>11.3f}   "
                     + " ".join(f"{x:.3f}" for x in v))
    lines.append("")
    verdicts = []
    for group in ("to host", "to device"):
        worst = max(s for (g, _), s in spread.items() if g == group)
        ok = med[group, "archive"] + worst < med[group, "containers"]
        verdicts.append(ok)
        lines.append(f"acceptance, {group}: median(archive) + largest spread of any variant ({worst:.3f} ms) < median(containers): "
                     f"{med[group, 'archive'] + worst:.3f} < {med[group, 'containers']:.3f} -> {'HOLDS' if ok else 'DOES NOT HOLD'}"
                     f"   (archive / containers = {med[group, 'archive'] / med[group, 'containers']:.2f})")
    for spec in a.kernel_trace:
        images, _, path = spec.partition("=")
        lines.append("")
        lines.append(f"kernels, from a profiler run of its own (rocprofv3 --kernel-trace --stats --output-format csv -- tools/ragged_archive_speed.py "
                     f"--only archive --calls {a.calls} --images {images}):")
        found = kernels_from_trace(path)
        moved = {"k_archive_copy<pack>": 2 * nbytes, "k_archive_copy<unpack>": 2 * nbytes} if int(images) == a.images else {}
        for kern, ns in sorted(found.items()):
            us = statistics.median(ns) / 1e3
            rate = f", {moved[kern]} bytes read + written = {moved[kern] / us / 1e6:.2f} TB/s (6.3 TB/s streaming)" if kern in moved else ""
            lines.append(f"  {kern:<24}{len(ns):6d} dispatches = {len(ns) / a.calls:.2f} per call, median {us:.2f} us "
                         f"(min {min(ns) / 1e3:.2f}, max {max(ns) / 1e3:.2f}){rate}")
        total = sum(len(v) for v in found.values())
        lines.append(f"  {'all':<24}{total:6d} dispatches = {total / a.calls:.2f} per pack + unpack (2 + 2 expected)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0 if equal else 2          # the verdict is a measurement, printed above; only unequal outputs are an error


if __name__ == "__main__":
    sys.exit(main())
