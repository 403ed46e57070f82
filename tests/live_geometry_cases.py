"""Weights, geometries and oracle outputs shared by tests/test_live_geometry_gpu.py, tests/test_live_geometry.py and the `--live` leg of
tests/fuzz_parity.py (no tests here).

A chain is a PRODUCER, conv or deconv 128 -> 128, followed by one or two CONSUMERS whose weights read only some of its channels: in a net
the producer is then neither last nor tapped and runs k_conv_live / k_deconv_live (csrc/k_mfma16x_live.hip) with 3 or 5 of its 8
accumulator columns.  The producer's weights do not depend on which channels are dead, so its oracle output is computed once per
geometry; a consumer of a given kind has the same weights at every width, with the dead input channels zeroed in every tap:
  80 dead = 48 live = 3 columns, every one of the 48 computed positions read;  48 dead = 80 live = 5 columns, all read;  0 dead = 8.
The oracle is c_oracle.run_layer in its direct form (integer: exact at 128 channels of bytes up to 255), one layer at a time."""
import functools

import numpy as np

from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import LayerDesc

N_DEAD = {3: 80, 5: 48, 8: 0}               # columns the producer runs -> dead input channels of its consumer
# kind: (cout, SIMD, PE, transposed)
KINDS = {"conv": (128, 8, 16, 0), "deconv": (128, 8, 16, 1), "rgb": (3, 8, 3, 1), "conv192": (192, 8, 24, 0)}
TILE_W, TILE_H = 32, 16                     # a wide kernel's tile of positions: conv outputs, deconv inputs (csrc/sicn_plan.h)


def desc(kind, w, h):
    cout, simd, pe, tr = KINDS[kind]
    return LayerDesc.make(128, cout, simd, pe, w, h, tr)


def chain_descs(kinds, w, h):
    """descriptors of `kinds` one behind the other, the first one on a w x h input"""
    out = []
    for k in kinds:
        out.append(desc(k, w, h))
        w, h = out[-1].OFM_ROW, out[-1].OFM_COL
    return out


def position_map(d):
    """(w, h) of the positions a wide kernel tiles: the conv's outputs, the deconv's inputs"""
    return (d.IFM_ROW, d.IFM_COL) if d.transposed else (d.OFM_ROW, d.OFM_COL)


def tiles(d):
    w, h = position_map(d)
    return (w + TILE_W - 1) // TILE_W, (h + TILE_H - 1) // TILE_H


@functools.lru_cache(maxsize=None)
def weights(kind, seed, n_dead=0):
    """(W[o][ky][kx][c] int8 in -8 .. 7, bias int8): W and the bias depend on (kind, seed) alone; n_dead random input channels, drawn
    from (seed, n_dead), are zero in every tap.  The bias differs per channel, so that one that did not follow its channel's
    permutation is readable."""
    cout = KINDS[kind][0]
    rng = np.random.default_rng([seed, sorted(KINDS).index(kind)])
    w = rng.integers(-8, 8, (cout, 5, 5, 128)).astype(np.int8)
    b = rng.integers(-128, 128, cout).astype(np.int8)
    if n_dead:
        w[:, :, :, dead_channels(seed, n_dead)] = 0
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


def dead_channels(seed, n_dead):
    return np.sort(np.random.default_rng([seed, 1000 + n_dead]).permutation(128)[:n_dead])


def live_channels(w):
    return np.flatnonzero(np.any(w != 0, axis=(0, 1, 2)))


def words(kind, w):
    _, simd, pe, _ = KINDS[kind]
    return sicn_ref.pack_finn_tiles(w, simd, pe)


def okc(w):
    """[cout][25 cin] with k = tap cin + c, as a weights handle keeps it on the host and tests/cpp/call_plan_check.cpp reads it"""
    return np.ascontiguousarray(w.reshape(w.shape[0], -1))


def images(seed, d, n):
    return np.random.default_rng([seed, 7]).integers(0, 256, (n,) + d.in_shape, dtype=np.uint8)


def oracle_layer(kind, d, wb, x):
    """every image of x [n][h][w][c] through one layer"""
    w, b = wb
    wd = words(kind, w)
    return np.stack([c_oracle.run_layer(d, wd, b, x[i], form="direct", threads=16) for i in range(len(x))])


_REF = {}


def reference(kinds, w, h, n, seed, n_dead):
    """outputs of every layer of the chain `kinds` on n seeded images of w x h, computed once and never changed.  Layer 0 is the producer
    (dense); layer l > 0 has n_dead dead input channels (weights and dead set of seed + l).  A prefix of a chain is shared by every
    chain that starts with it: the producer's output is computed once per geometry whatever the width and the consumer."""
    descs = chain_descs(kinds, w, h)
    x = images(seed, descs[0], n)
    outs = []
    for l, (k, d) in enumerate(zip(kinds, descs)):
        key = (tuple(kinds[:l + 1]), w, h, n, seed, n_dead if l else 0)
        if key not in _REF:
            y = oracle_layer(k, d, chain_weights(kinds, seed, n_dead)[l], x)
            y.setflags(write=False)
            _REF[key] = y
        x = _REF[key]
        outs.append(x)
    return outs


def chain_weights(kinds, seed, n_dead):
    return [weights(k, seed + l, n_dead if l else 0) for l, k in enumerate(kinds)]
