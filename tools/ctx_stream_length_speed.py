#!/usr/bin/env python3
"""What the stream length of the rANS-WC coder buys and costs (profiles/ctx_stream_length_speed.txt).

For every stream length S in 16384, 8192, 4096, 2048, 1024 (codec.RaggedContextCoder(..., stream_symbols=S)), on the latents and scale
maps of hyperprior.RaggedHyperpriorCodec, made once, before timing:
  one       one 640 x 640 image: y container bytes, encode and decode time
  mix       the seeded mix of 64 image sizes of tools/ragged_hyper_speed.py: the same
  roi x 1   the window decoder over the latent rows of the centred 256 x 256 rectangle of a 640 x 640 image (api.roi_plan): selected
  roi x 4   streams, band rows and the time of codec.RaggedContextWindowDecoder.decode — one image, and four of them

Method: every object is made before timing and warmed up; the lengths ALTERNATE in one process for --rounds rounds, each timed with
device events around enough back-to-back repetitions to fill --seconds; after every timed call of every round the decoded latents are
compared with the input (the containers of one length with those of the first round).  Reported: median over the rounds and the spread
(max - min).

  python tools/ctx_stream_length_speed.py                          the table
  python tools/ctx_stream_length_speed.py --json --lengths 1024 --what mix      one JSON line (for alternating two builds of the library,
                                                                                 chosen with SICN_LIB, from a shell loop)
  python tools/ctx_stream_length_speed.py --only roi1 --lengths 1024 --calls 20      just that, for a profiler run of its own:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ctx_stream_length_speed.py --only roi1 --lengths 1024 --calls 20
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from ragged_speed import make_sizes  # noqa: E402  (the same seeded mix)

LENGTHS = [16384, 8192, 4096, 2048, 1024]
ROI = (192, 192, 256, 256)                                   # the centred 256 x 256 rectangle of a 640 x 640 image


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.25)
    ap.add_argument("--lengths", type=int, nargs="+", default=LENGTHS)
    ap.add_argument("--what", nargs="+", choices=["one", "mix", "roi1", "roi4"], default=["one", "mix", "roi1", "roi4"])
    ap.add_argument("--only", choices=["one", "mix", "roi1", "roi4"], help="run the decode of that workload --calls times and exit")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--json", action="store_true", help="one JSON line instead of the table")
    ap.add_argument("--out", help="also write the table to this file")
    a = ap.parse_args()
    if a.rounds < 3 and not a.only:
        ap.error("--rounds: at least 3")
    what = [a.only] if a.only else a.what

    import numpy as np
    import torch

    from simple_image_compression_network_amd import _lib, api, codec, hyperprior

    L = _lib.lib()
    chip = (ctypes.c_int32 * 2)()
    _lib.check(L.sicn_debug_chip(chip), "sicn_debug_chip")
    n_cu = int(chip[0])
    workloads = {"one": [(640, 640)], "mix": make_sizes(a.seed, a.images), "roi1": [(640, 640)], "roi4": [(640, 640)] * 4}
    params = api.load_param_weights()
    rng = np.random.default_rng(a.seed + 1)

    def latents(sizes):
        images = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for w, h in sizes]
        hc = hyperprior.RaggedHyperpriorCodec(sizes, seed=a.seed, main_params=params)
        hc.main.run_layers(0, 3, hc.main.pack(images), out=hc.y)
        hc.h_a.run_layers(0, 1, hc.y, out=hc.z)
        hc._scale_map(hc.z)
        torch.cuda.synchronize()
        return hc.y.clone(), hc.s.clone(), hc.main.shapes(3)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3                # us

    results, lines, equal_all = {}, [], True
    for name in what:
        sizes = workloads[name]
        y, s, shapes = latents(sizes)
        hw = [(h, w) for h, w, _ in shapes]
        c = shapes[0][2]
        symbols = sum(h * w * ch for h, w, ch in shapes)
        coders, wins, backs, info = {}, {}, {}, {}
        for S in a.lengths:                                    # every object before timing
            coder = codec.RaggedContextCoder(hw, c, sizes, stream_symbols=S)
            coders[S] = coder
            backs[S] = torch.empty_like(y)
            info[S] = {"streams": sum(int(im.anchor_streams) + int(im.nonanchor_streams) for im in coder.images[:len(hw)])}
            if name.startswith("roi"):
                plans = [api.roi_plan(size, ROI) for size in sizes]
                win = coder.window([(p["r0"], p["rh"]) for p in plans])
                wins[S] = (win, torch.empty(win.band_bytes, dtype=torch.uint8, device="cuda"), plans)
                info[S].update(selected=win.selected_streams, band_rows=int(win.images[0].band_rows), wanted_rows=plans[0]["rh"])
        fns = {}
        for S in a.lengths:
            coder = coders[S]
            fns[(S, "enc")] = (lambda coder=coder: coder.encode(y, s))
            if name.startswith("roi"):
                win, band, _ = wins[S]
                fns[(S, "dec")] = (lambda win=win, band=band: win.decode(band, s))
            else:
                fns[(S, "dec")] = (lambda coder=coder, S=S: coder.decode(backs[S], s))

        def verify(S):
            coder = coders[S]
            torch.cuda.synchronize()
            coder.check()
            if name.startswith("roi"):
                win, band, plans = wins[S]
                win.check()
                ok = True
                for v, p, full in zip(win.views(band), plans, coder.views(y)):
                    ok &= torch.equal(v, full[p["r0"]:p["r0"] + p["rh"]])
                return ok
            return torch.equal(backs[S], y)

        for S in a.lengths:                                    # warm-up, and the first round's containers
            fns[(S, "enc")](); fns[(S, "enc")](); fns[(S, "dec")](); fns[(S, "dec")]()
            equal_all &= verify(S)
            info[S]["bytes"] = sum(coders[S].sizes())
            info[S]["containers"] = coders[S].slot_buffer.clone()
        if a.only:
            S = a.lengths[0]
            for _ in range(a.calls):
                fns[(S, "dec")]()
            torch.cuda.synchronize()
            print(f"{a.only} at {S}: {a.calls} decode calls done")
            return 0
        reps = {k: max(2, int(a.seconds * 1e6 / timed(fn, 3)) + 1) for k, fn in fns.items()}
        us = {k: [] for k in fns}
        for _ in range(a.rounds):
            for S in a.lengths:                                # the lengths alternate inside a round
                for d in ("enc", "dec"):
                    us[(S, d)].append(timed(fns[(S, d)], reps[(S, d)]))
                equal_all &= verify(S) and torch.equal(coders[S].slot_buffer, info[S]["containers"])
        base = info[a.lengths[0]]
        lines.append(f"--- {name}: {len(sizes)} image(s), {symbols / 1e6:.2f} M symbols" + (f"; rows wanted {base['wanted_rows']}" if "wanted_rows" in base else ""))
        lines.append(f"{'S':>6}{'streams':>9}{'y bytes':>11}{'+ % bytes':>10}{'B/stream':>9}"
                     + (f"{'selected':>9}{'band rows':>10}" if name.startswith("roi") else "")
                     + f"{'enc us':>10}{'spread':>8}{'dec us':>10}{'spread':>8}   rounds enc | dec (us)")
        for S in a.lengths:
            i = info[S]
            e, d = us[(S, "enc")], us[(S, "dec")]
            extra = i["bytes"] - base["bytes"]
            per_stream = extra / (i["streams"] - base["streams"]) if i["streams"] != base["streams"] else 0.0
            lines.append(f"{S:>6}{i['streams']:>9}{i['bytes']:>11}{100 * extra / base['bytes']:>10.2f}{per_stream:>9.0f}"
                         + (f"{i['selected']:>9}{i['band_rows']:>10}" if name.startswith("roi") else "")
                         + f"{statistics.median(e):>10.1f}{max(e) - min(e):>8.1f}{statistics.median(d):>10.1f}{max(d) - min(d):>8.1f}   "
                         + " ".join(f"{v:.1f}" for v in e) + " | " + " ".join(f"{v:.1f}" for v in d))
            results[f"{name}:{S}"] = {"enc_us": e, "dec_us": d, "bytes": i["bytes"], "streams": i["streams"]}
        lines.append("")
    head = [f"tools/ctx_stream_length_speed.py --seed {a.seed} --images {a.images} --rounds {a.rounds} --seconds {a.seconds}",
            f"device: {torch.cuda.get_device_name(0)}, {n_cu} CUs; library {_lib.LIB_PATH.name}; 'dec' of the roi rows is the window decoder's call",
            f"decoded latents (roi: the wanted rows) equal the input, and containers equal the first round's, after every timed call: {equal_all}", ""]
    text = "\n".join(head + lines)
    if a.json:
        print(json.dumps({"lib": str(_lib.LIB_PATH), "equal": bool(equal_all), "results": results}))
    else:
        print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0 if equal_all else 2


if __name__ == "__main__":
    sys.exit(main())
