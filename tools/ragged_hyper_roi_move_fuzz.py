#!/usr/bin/env python3
"""Randomised sweep of the hyperprior moving ROI decode (hyperprior.MovingHyperpriorRoi) in the style of tests/fuzz_parity.py: random
batches of image sizes, random y stream lengths, random slots and random positions — a few of them outside the image — against the
codec's own full decode() + main.cropped, sliced in numpy, byte for byte; flags against the clamp.  A tool, not a test: needs a GPU.

  python tools/ragged_hyper_roi_move_fuzz.py [--cases N] [--moves M] [--seed S] [--max-side PIXELS]
Exit status 0 when every move of every case was equal."""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", type=int, default=20)
    ap.add_argument("--moves", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-side", type=int, default=400)
    a = ap.parse_args()

    import torch

    from simple_image_compression_network_amd import hyperprior

    rng = np.random.default_rng(a.seed)
    bad = moves = 0
    for case in range(a.cases):
        n = int(rng.integers(1, 6))
        sizes = [(int(rng.integers(1, a.max_side + 1)), int(rng.integers(1, a.max_side + 1))) for _ in range(n)]
        wss = [int(2 ** rng.integers(10, 15)) for _ in range(n)]
        use_gdn = bool(rng.integers(2))
        rc = hyperprior.RaggedHyperpriorCodec(sizes, seed=int(rng.integers(1 << 16)), use_gdn=use_gdn, y_stream_symbols=wss)
        rc.encode(rc.main.pack([torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in sizes]))
        full = rc.decode()
        rc.check()
        want = [v.cpu().numpy() for v in rc.main.crop_views(rc.main.cropped(full))]
        slots = []
        for _ in range(int(rng.integers(1, 9))):
            i = int(rng.integers(n))
            whole = rng.random() < 0.15
            slots.append((i, sizes[i][0] if whole else int(rng.integers(1, sizes[i][0] + 1)), sizes[i][1] if whole else int(rng.integers(1, sizes[i][1] + 1))))
        mv = rc.moving_roi(slots)
        mv.prepare()
        for move in range(a.moves):
            xy = []
            for i, w, h in slots:
                x, y = int(rng.integers(0, sizes[i][0] - w + 1)), int(rng.integers(0, sizes[i][1] - h + 1))
                if rng.random() < 0.1:
                    x = int(rng.choice([-1, -2 ** 31, 2 ** 31 - 1, sizes[i][0] - w + 1]))
                if rng.random() < 0.1:
                    y = int(rng.choice([-1, -2 ** 31, 2 ** 31 - 1, sizes[i][1] - h + 1]))
                xy.append((x, y))
            out = mv.decode(xy)
            torch.cuda.synchronize()
            status, flags = mv.status[:, 0].cpu().tolist(), mv.flags.cpu().tolist()
            moves += 1
            for k, ((i, w, h), (x, y), v) in enumerate(zip(slots, xy, mv.views(out))):
                cx, cy = min(max(x, 0), sizes[i][0] - w), min(max(y, 0), sizes[i][1] - h)
                ok = status[k] == 0 and flags[k] == int((cx, cy) != (x, y)) and np.array_equal(v.cpu().numpy(), want[i][cy:cy + h, cx:cx + w])
                if not ok:
                    bad += 1
                    print(f"case {case} move {move} slot {k}: sizes {sizes} symbols {wss} gdn {use_gdn} slots {slots} xy {xy} status {status[k]} "
                          f"flags {flags[k]}: MISMATCH")
        print(f"case {case}: {n} images {sizes}, y streams {wss}, gdn {use_gdn}, {len(slots)} slots, work items {mv.items}: {a.moves} moves", flush=True)
    print(f"{a.cases} cases, {moves} moves, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
