"""Weights, geometries and oracle outputs shared by tests/test_l0_live_groups_gpu.py and tests/test_l0_live_groups.py (no tests here).

The nets are the first two or three layers of the reference's net, `eight_layer_descs(w, h)[:2]` and `[:3]`: layer 0 (conv 3 -> 128,
"l0_rgb"), layer 1 (conv 128 -> 128) and layer 2 (the same).  A weight set is the PARAM fixture (48 dead input channels in layers 1 and
2, c mod 8 >= 5) or seeded random weights whose layer-1 input has 48, 32, 31 or 0 dead channels, drawn at random:
  48 and 32 dead: layer 0 computes and stores three of its four 32-channel groups (80 and 96 live channels, csrc/sicn_live.h);
  31 and 0 dead : the controls, all four groups: they tell a fault of the test from a fault of the three-group kernel.
Layer 2 of a random set always has 48 dead input channels, so that layer 1 of a `[:3]` net runs 5 accumulator columns and takes the
copy of its weights that is permuted on both sides (behind three groups) or on the output side alone (behind four).
The oracle is c_oracle.run_layer in its direct form (integer: exact), one layer at a time, every output computed once."""
import functools
from pathlib import Path

import numpy as np

from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import NET_CHANNELS, eight_layer_descs

GOLDEN = Path(__file__).resolve().parent / "golden" / "param_weights.npz"
SEED = 31
SETS = {"param": 48, "r48": 48, "r32": 32, "r31": 31, "r0": 0}     # weight set -> dead input channels of layer 1
L2_DEAD = 48
L0_TILE_W, L0_TILE_H = 32, 8                 # k_l0's tile of output positions (csrc/sicn_plan.h: TILE_X, L0_TY)


def groups(wset):
    """the groups layer 0 runs where it is neither last nor tapped"""
    return 3 if 128 - SETS[wset] <= 96 else 4


def descs(w, h, n_layers):
    return eight_layer_descs(w, h)[:n_layers]


def dead_channels(wset, layer):
    n_dead = SETS[wset] if layer == 1 else L2_DEAD
    return np.sort(np.random.default_rng([SEED, 1000 * layer + n_dead]).permutation(128)[:n_dead])


@functools.lru_cache(maxsize=None)
def _param():
    return sicn_ref.load_param_fixture(GOLDEN)


@functools.lru_cache(maxsize=None)
def weights(wset, layer):
    """(W[o][ky][kx][c] int8 in -8 .. 7, bias int8) of layer 0, 1 or 2.  Random sets: layer 0 and the non-zero weights of layers 1, 2
    depend on the layer alone, the dead channels on the set; the bias differs per channel, so that one that did not follow its
    channel's permutation is readable."""
    if wset == "param":
        w, b, _ = _param()[layer]
        w, b = w.astype(np.int8), b.astype(np.int8)
    else:
        cin, cout = NET_CHANNELS[layer][:2]
        rng = np.random.default_rng([SEED, layer])
        w = rng.integers(-8, 8, (cout, 5, 5, cin)).astype(np.int8)
        b = rng.integers(-128, 128, cout).astype(np.int8)
        if layer:
            w[:, :, :, dead_channels(wset, layer)] = 0
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


def live_channels(w):
    return np.flatnonzero(np.any(w != 0, axis=(0, 1, 2)))


def words(layer, w):
    _, _, simd, pe, _ = NET_CHANNELS[layer]
    return sicn_ref.pack_finn_tiles(w, simd, pe)


def okc(w):
    return np.ascontiguousarray(w.reshape(w.shape[0], -1))


def images(w, h, n):
    return np.random.default_rng([SEED, 7, w, h]).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def oracle_layer(layer, d, wb, x):
    w, b = wb
    wd = words(layer, w)
    return np.stack([c_oracle.run_layer(d, wd, b, x[i], form="direct", threads=16) for i in range(len(x))])


_REF = {}


def reference(wset, w, h, n, n_layers):
    """outputs of the layers 0 .. n_layers - 1 on n seeded images of w x h, computed once and never changed; layer 0 of every random
    set is the same layer, and a `[:2]` net shares its outputs with the `[:3]` net"""
    x = images(w, h, n)
    outs = []
    for l, d in enumerate(descs(w, h, n_layers)):
        key = (wset if (l or wset == "param") else "random", l, w, h, n)
        if key not in _REF:
            y = oracle_layer(l, d, weights(wset, l), x)
            y.setflags(write=False)
            _REF[key] = y
        x = _REF[key]
        outs.append(x)
    return outs
