#!/usr/bin/env python3
"""Speed of the generic ConvLayer with resident parameters (convlayer.ConvLayer): the automatic kernel choice (kernel=0)
against the direct kernel (kernel=1), on quantised layers with sub-byte lanes and on the byte-lane shapes of tools/convlayer_speed.py.
Device events around 20 launches after a warm-up; the two kernels alternate, each timed `--rounds` times.  Operations = 2 x the layer's
multiply-accumulates over its real channels (int8 operations), reported as TOP/s and as a share of the int8 MFMA peak."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from simple_image_compression_network_amd import api, convlayer as cl  # noqa: E402

INT8_PEAK = 5.0e15      # MI355X dense int8 MFMA (spec; 2x the BF16 rate per clock)

# (name, K, C, D, O, reps, IN_BIT, OUT_BIT, NUM_TH, W_BIT)
LOWBIT = [
    ("CNV-style 2-bit in, 3 thresholds, 2-bit out", 3, 64, 32, 64, 256, 2, 2, 3, 2),
    ("4-bit in, 15 thresholds, 4-bit out", 3, 256, 66, 256, 8, 4, 4, 15, 4),
    ("3-channel 8-bit first layer, 3 thresholds, 2-bit out", 3, 3, 130, 64, 64, 8, 2, 3, 4),
]
BYTE = [(f"byte lanes (tools/convlayer_speed.py), 32-bit out", K, C, D, O, reps, 8, 32, 0, 4)
        for (K, C, D, O, reps) in [(3, 64, 130, 64, 4), (5, 128, 68, 128, 4), (1, 256, 64, 256, 4), (3, 16, 258, 32, 4)]]


def make_layer(rng, K, C, D, O, IB, OB, NTH, WB):
    simd = max(s for s in (1, 2, 3, 4, 8) if C % s == 0 and s * WB <= 64)
    pe = min(O, 8)
    desc = cl.ConvLayerDesc(K=K, IFM_CH=C, IFM_DIM=D, OFM_CH=O, SIMD=simd, PE=pe, W_BIT=WB, IN_SIGNED=False, OUT_BIT=OB, IN_BIT=IB)
    w = rng.integers(-(1 << (WB - 1)), 1 << (WB - 1), (O, K * K * C)).astype(np.int64)
    nf, sf = O // pe, K * K * C // simd
    el = (w.reshape(nf, pe, sf, simd) & ((1 << WB) - 1)).astype(np.uint64)
    words = (el << (np.arange(simd, dtype=np.uint64) * np.uint64(WB))[None, None, None, :]).sum(axis=3, dtype=np.uint64)
    words = np.ascontiguousarray(words.transpose(1, 0, 2).reshape(pe, nf * sf))
    fpw = api.FixedPointWeights(simd, WB, pe, desc.W_TILES, words)
    if NTH:
        span = int(3 * (1 << (WB - 1)) * (1 << IB) * np.sqrt(K * K * C))
        thr = np.sort(rng.integers(-span, span, (pe, O // pe, NTH)), axis=2).astype(np.int32)
        act = cl.ThresholdsActivation(thr, ACC_BIT=24, ACC_SIGNED=True, ACT_VAL=0)
    else:
        act = cl.PassThroughActivation(ACC_BIT=32, ACC_SIGNED=True)
    return cl.ConvLayer(desc, fpw, act)


def time_us(layer, x, out, reps, kernel, n=20):
    for _ in range(3):
        layer(x, out, reps, kernel=kernel)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        layer(x, out, reps, kernel=kernel)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--byte-only", action="store_true", help="only the byte-lane shapes of tools/convlayer_speed.py")
    ap.add_argument("--no-direct", action="store_true", help="time the automatic choice only")
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    kernels = [0] if a.no_direct else [0, 1]
    print(f"# {torch.cuda.get_device_name(0)}; events around 20 launches after 3 warm-up launches; AUTO and DIRECT alternate, "
          f"{a.rounds} rounds; TOP/s = 2 x real MACs / time; % of int8 MFMA peak {INT8_PEAK / 1e15:.1f} POP/s")
    for (name, K, C, D, O, reps, IB, OB, NTH, WB) in (BYTE if a.byte_only else LOWBIT + BYTE):
        layer = make_layer(rng, K, C, D, O, IB, OB, NTH, WB)
        shape_in, _, _ = layer.shapes(reps)
        x = torch.from_numpy(rng.integers(0, 256, shape_in, dtype=np.uint8)).cuda()
        outs = {k: layer(x, None, reps, kernel=k) for k in kernels}
        torch.cuda.synchronize()
        same = "" if len(kernels) == 1 else f"; AUTO bytes == DIRECT bytes: {torch.equal(outs[0], outs[1])}"
        times = {k: [] for k in kernels}
        for _ in range(a.rounds):
            for k in kernels:
                times[k].append(time_us(layer, x, outs[k], reps, k))
        ops = 2.0 * reps * layer.desc.OFM_DIM ** 2 * O * K * K * C
        print(f"{K}x{K}x{C}->{O} IN_BIT={IB} OUT_BIT={OB} NUM_TH={NTH} on {reps} x {D}^2 ({name}); AUTO = {getattr(layer, 'kernel', '?')}{same}")
        for k in kernels:
            t = min(times[k])
            print(f"    {'AUTO  ' if k == 0 else 'DIRECT'} {t:10.1f} us (rounds: {', '.join(f'{v:.1f}' for v in times[k])})  "
                  f"{ops / t / 1e6:8.2f} TOP/s  {100 * ops / t / 1e-6 / INT8_PEAK:6.2f} % of int8 peak")
        layer.close()


if __name__ == "__main__":
    main()
