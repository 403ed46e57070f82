"""The sweep of call plans behind tests/test_call_plan_gpu.py and tests/golden/call_plans.json (no tests here).

What a call of a net does with each of its layers — the columns and groups it computes, the groups behind its input, the halves and
groups of its input it reads, the output channels somebody reads — is asked of the library through the four sicn_debug_net_* entry
points, and the kernel kind and MFMA family of every layer through sicn_debug_plan; no layer is launched.  The net handles need a device
for their weight uploads.  `python tests/call_plan_cases.py OUT.json` records the sweep in the fixture's form.

The nets, each as 8 layers and as 3:
  * tests/l0_groups_cases.py: the PARAM weights, and random weights with 48, 32, 31 and 0 dead layer-1 inputs;
  * tests/live_geometry_cases.py: chains of 128 -> 128 layers in front of the RGB deconv whose consumers read 48 channels (3 columns);
  * the PARAM weights with a GDN on layer 1.
Each is swept over every [first, last], tap_layer in {-1, first, 3 if in range, last}, 1 and 3 images and the options wave_tile = 128,
wave_tile = 64, force_generic = 1 and the defaults; the images are 14 x 10, far below every automatic threshold, so that no answer depends
on the chip.

A record is one digit string: per layer `cols halves groups groups_in walk` (one digit each) and the live outputs (three digits).  The
fixture holds every different string once (`strings`) and the sweep's records as indices into them, in the order of records()."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))

import l0_groups_cases as gc  # noqa: E402
import live_geometry_cases as lg  # noqa: E402
from simple_image_compression_network_amd import _lib, api  # noqa: E402
from simple_image_compression_network_amd.config import eight_layer_descs  # noqa: E402

FIXTURE = ROOT / "tests" / "golden" / "call_plans.json"
W, H = 14, 10
N_CU = 256                                   # sicn_debug_plan's chip: nothing in the sweep depends on it
OPTIONS = [{"wave_tile": 128}, {"wave_tile": 64}, {"force_generic": 1}, {}]
N_IMAGES = (1, 3)
CHAINS = {8: ("conv", "conv", "conv", "deconv", "deconv", "deconv", "deconv", "rgb"), 3: ("deconv", "deconv", "rgb")}
CHAIN_SEED, CHAIN_DEAD = 77, lg.N_DEAD[3]


def _gdn():
    rng = np.random.default_rng(9)
    return api.GDN(rng.integers(1, 65536, 128).astype(np.uint32), rng.integers(0, 128, (128, 128)).astype(np.uint8))


def nets():
    """(name, descriptors, [(FixedPointWeights, bias)], gdn list or None) of every net of the sweep"""
    for n_layers in (8, 3):
        descs = eight_layer_descs(W, H)[:n_layers]
        for wset in gc.SETS:
            params = [(api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, gc.words(l, gc.weights(wset, l)[0])), gc.weights(wset, l)[1])
                      for l, d in enumerate(descs)]
            yield f"{wset}-{n_layers}", descs, params, None
            if wset == "param":
                yield f"param-gdn1-{n_layers}", descs, params, [None, _gdn()] + [None] * (n_layers - 2)
        kinds = CHAINS[n_layers]
        descs = lg.chain_descs(kinds, W, H)
        params = [(api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, lg.words(k, w)), b)
                  for k, d, (w, b) in zip(kinds, descs, lg.chain_weights(kinds, CHAIN_SEED, CHAIN_DEAD))]
        yield f"chain-{n_layers}", descs, params, None


def calls(n_layers):
    for first in range(n_layers):
        for last in range(first, n_layers):
            taps = [-1, first] + ([3] if first <= 3 <= last else []) + [last]
            for tap in sorted(set(taps)):
                yield first, last, tap


def _ints(fn, net, first, last, tap, n, count):
    arrays = [(ctypes.c_int32 * 64)() for _ in range(count)]
    _lib.check(getattr(_lib.lib(), fn)(net._h, first, last, tap, n, *arrays), fn)
    return [list(a)[:len(net.descs)] for a in arrays]


def records():
    """(key, digit string) of the whole sweep, in a fixed order"""
    for name, descs, params, gdn in nets():
        weights = [api.DeviceWeights(d, w, b) for d, (w, b) in zip(descs, params)]
        for options in OPTIONS:
            oname = ",".join(f"{k}={v}" for k, v in options.items()) or "defaults"
            net = api.EightLayersNet(descs=descs, shared_weights=weights, options=options, gdn=gdn)
            for n in N_IMAGES:
                plan = (ctypes.c_int32 * 12)()
                kinds = ""
                for d in descs:
                    _lib.check(_lib.lib().sicn_debug_plan(ctypes.byref(d.to_c()), n, ctypes.byref(_lib.make_options(**options)), N_CU, plan),
                               "sicn_debug_plan")
                    kinds += f"{plan[2]}{plan[3]}"
                yield f"{name} {oname} n{n} kinds", kinds
                for first, last, tap in calls(len(descs)):
                    cols, live = _ints("sicn_debug_net_columns", net, first, last, tap, n, 2)
                    halves, = _ints("sicn_debug_net_input_halves", net, first, last, tap, n, 1)
                    groups, groups_in = _ints("sicn_debug_net_groups", net, first, last, tap, n, 2)
                    walk, = _ints("sicn_debug_net_walk_groups", net, first, last, tap, n, 1)
                    yield (f"{name} {oname} n{n} [{first}, {last}] tap {tap}",
                           "".join(f"{c}{h}{g}{gi}{wk}{lv:03d}" for c, h, g, gi, wk, lv in zip(cols, halves, groups, groups_in, walk, live)))


def pack(recs):
    strings, sweep = {}, []
    for _, s in recs:
        sweep.append(strings.setdefault(s, len(strings)))
    return {"strings": list(strings), "sweep": sweep}


if __name__ == "__main__":
    out = pack(records())
    Path(sys.argv[1]).write_text(json.dumps(out, separators=(",", ":")) + "\n")
    print(f"{len(out['sweep'])} records, {len(out['strings'])} different")
