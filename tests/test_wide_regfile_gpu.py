"""The wide persistent kernels (k_conv_x / k_deconv_x, csrc/k_mfma16x.hip) spread their accumulator columns, the columns' bias and their
operand fragments over both register files (k_deconv_x: fragments in AGPRs, most accumulator columns in VGPRs).  The parity tests of test_gpu_parity.py / test_gdn.py hold every byte of these kernels to the oracle with random
weights; the cases here use weights that make the two mistakes such a register map can make READABLE:
  * a bias register in the wrong file / column (the first pass of a tile takes the bias as its C operand, through either file),
  * a swapped or stale operand fragment (one ds_read_b128 into four AGPRs per fragment, read by the MFMAs one pass later),
and they run the identity floor of the hand-over's pack (the lane in front of the GDN extension) with half of the lanes negative.
wave_tile = 128, persistent_grid = 8 and 3 images throughout: 2 x 2 tiles per image = 12 tiles on 8 workgroups, so both the first-tile
path (accumulators initialised by moves) and the hand-over path (C = bias in the next tile's first pass) are taken."""
import numpy as np
import pytest

from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import LayerDesc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OPTIONS = {"wave_tile": 128, "persistent_grid": 8}
N_IMG = 3
# (input width, input height, transposed): conv 66 x 34 -> 33 x 17 outputs, deconv 33 x 17 inputs: 2 x 2 tiles of 16 x 32 positions
SHAPES = [(66, 34, 0), (33, 17, 1)]
RAGGED = [(70, 45, 0), (35, 21, 1)]
TY, TX = 16, 32


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import api as _api
    return _api


def _desc(w, h, transposed):
    return LayerDesc.make(128, 128, 8, 16, w, h, transposed)


def _run(api, d, W, b, x, gdn=None):
    fpw = api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, sicn_ref.pack_finn_tiles(W, d.SIMD, d.PE))
    fn = api.deconv522 if d.transposed else api.conv2d
    out = fn(d, fpw, b, torch.from_numpy(np.ascontiguousarray(x)).cuda(), None, x.shape[0], gdn=gdn, options=OPTIONS)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _lane_layout(c):
    """channel c = 64 (j >> 2) + 16 g + 4 (j & 3) + r -> (accumulator column j, register r, lane group g)"""
    return 4 * (c >> 6) + ((c >> 2) & 3), c & 3, (c >> 4) & 3


def _where(d, y, x, c):
    """where output byte (y, x, c) sits in the kernel's walk: tile-local (row, 16-position column block) of the M grid, the deconv's
    phase, and the accumulator column / register of the channel"""
    my, mx = (y >> 1, x >> 1) if d.transposed else (y, x)
    j, r, g = _lane_layout(c)
    s = f"tile ({my // TY}, {mx // TX}) row {my % TY} column block {(mx % TX) // 16} position {mx % 16}"
    if d.transposed:
        s += f" phase ({y & 1}, {x & 1})"
    return s + f"; channel {c} = accumulator column j {j}, register r {r}, lane group g {g}"


def _inputs(rng, d):
    x = rng.integers(0, 128, (N_IMG,) + d.in_shape, dtype=np.uint8)
    x[0].reshape(-1)[::7] |= 0x80
    return x


@pytest.mark.parametrize("shape", SHAPES, ids=["conv66x34", "deconv33x17"])
def test_bias_on_its_own_channel(api, shape):
    """Weights zero, b[c] = (37 c + 11) mod 128 (a permutation of 0 .. 127, which the ReLU keeps): every output pixel must be b."""
    d = _desc(*shape)
    W = np.zeros((128, 5, 5, 128), np.int8)
    b = ((37 * np.arange(128) + 11) % 128).astype(np.int8)
    assert sorted(b.tolist()) == list(range(128))
    x = _inputs(np.random.default_rng(11 + shape[2]), d)
    got = _run(api, d, W, b, x)
    ref_fn = sicn_ref.deconv522_ref if d.transposed else sicn_ref.conv2d_ref
    for i in range(N_IMG):
        ref = ref_fn(x[i], W, b)
        assert np.array_equal(ref, np.broadcast_to(b.astype(np.uint8), ref.shape))   # what the oracle says is what the docstring says
        if not np.array_equal(got[i], ref):
            bad = np.argwhere(got[i] != ref)
            chans = sorted({int(c) for c in bad[:, 2]})
            y, xx, c = (int(v) for v in bad[0])
            raise AssertionError(
                f"image {i}: {len(bad)} wrong bytes in {len(chans)} channels; wrong (column j, register r): "
                f"{sorted({_lane_layout(c)[:2] for c in chans})}; first: got {got[i][y, xx, c]} want {ref[y, xx, c]} at {_where(d, y, xx, c)}")


def _one_hot_weights():
    """W[c, ky(c), kx(c), p(c)] = 1: output channel c copies input channel p(c) of ONE tap, the tap cycling through all 25 positions
    over c (every pass of either kernel's walk carries weight), p a fixed permutation"""
    W = np.zeros((128, 5, 5, 128), np.int8)
    c = np.arange(128)
    p = (53 * c + 7) % 128
    assert sorted(p.tolist()) == list(range(128))
    W[c, (c % 25) // 5, (c % 25) % 5, p] = 1
    return W


@pytest.mark.parametrize("shape", SHAPES + RAGGED, ids=["conv66x34", "deconv33x17", "conv70x45", "deconv35x21"])
def test_every_fragment_register_on_its_own(api, shape):
    """One-hot weights: each output byte is one input byte (+ bias), so a swapped or stale A / B fragment shows as a permuted channel
    block or a shifted group of 16 positions instead of noise."""
    d = _desc(*shape)
    W = _one_hot_weights()
    rng = np.random.default_rng(23 + shape[0])
    b = rng.integers(0, 4, 128).astype(np.int8)
    x = _inputs(rng, d)
    got = _run(api, d, W, b, x)
    ref_fn = sicn_ref.deconv522_ref if d.transposed else sicn_ref.conv2d_ref
    for i in range(N_IMG):
        ref = ref_fn(x[i], W, b)
        if not np.array_equal(got[i], ref):
            bad = np.argwhere(got[i] != ref)
            y, xx, c = (int(v) for v in bad[0])
            raise AssertionError(f"image {i}: {len(bad)} wrong bytes, in accumulator columns {sorted({_lane_layout(int(c))[0] for c in bad[:, 2]})}; "
                                 f"first: got {got[i][y, xx, c]} want {ref[y, xx, c]} at {_where(d, y, xx, c)} "
                                 f"(tap ({(c % 25) // 5}, {(c % 25) % 5}), input channel {(53 * c + 7) % 128})")


@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
@pytest.mark.parametrize("shape", SHAPES, ids=["conv66x34", "deconv33x17"])
def test_identity_floor_keeps_negative_lanes(api, shape, inverse):
    """A GDN behind the layer makes the hand-over pack with the identity floor (-128): the lanes reach the activation unclipped.
    One-hot weights against inputs 0 .. 127, with biases in -128 .. -1 (conv) / -64 .. 63 (deconv, where three of four output phases
    of a channel see no tap and the lane is the bias itself): about half of the lanes are negative."""
    d = _desc(*shape)
    W = _one_hot_weights()
    rng = np.random.default_rng(31 + 2 * shape[2] + inverse)
    b = (rng.integers(-64, 64, 128) if d.transposed else rng.integers(-128, 0, 128)).astype(np.int8)
    x = rng.integers(0, 128, (N_IMG,) + d.in_shape, dtype=np.uint8)
    beta = rng.integers(1, 65536, 128).astype(np.uint32)
    gamma = rng.integers(0, 128, (128, 128)).astype(np.uint8)
    gamma[rng.random((128, 128)) < 0.5] = 0
    got = _run(api, d, W, b, x, gdn=api.GDN(beta, gamma, inverse, 12))
    for i in range(N_IMG):
        pre = sicn_ref.layer_preact_ref(x[i], W, b, d.transposed)
        neg = np.count_nonzero(pre >= 128) / pre.size
        assert 0.25 < neg < 0.75, neg   # the case is what it claims to be
        ref = c_oracle.gdn(pre, beta, gamma, inverse, 12)
        if not np.array_equal(got[i], ref):
            bad = np.argwhere(got[i] != ref)
            y, xx, c = (int(v) for v in bad[0])
            raise AssertionError(f"image {i}: {len(bad)} wrong bytes; first: got {got[i][y, xx, c]} want {ref[y, xx, c]} "
                                 f"(lane before the activation {pre[y, xx, c]}) at {_where(d, y, xx, c)}")
