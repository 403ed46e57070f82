"""ConvLayer_Batch on the int8 MFMA kernel for every layer shape (k_convlayer_patch): sub-byte input lanes, 2- / 4-bit
output lanes, any channel count.  The automatic choice (`kernel=0`) is compared byte for byte with the direct kernel (`kernel=1`) and,
through the independent Python restatement of the stream packing (sicn_ref.pack_stream_lanes / unpack_stream_lanes), with the restated
dataflow (oracle.c_oracle.convlayer_dataflow)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import c_oracle, sicn_ref
from test_convlayer import CASES, PACKED_CASES

MFMA = "k_convlayer_patch"

# (K, C, D, O, SIMD, PE, W_BIT, IN_BIT, IN_SIGNED, ACC_BIT, ACC_SIGNED, OUT_BIT, NUM_TH, ACT_VAL); a tile is 16 x 16 output positions
GRID = [
    (3, 8, 20, 8, 4, 2, 4, 1, 0, 16, 1, 2, 3, -1),          # binary lanes in, 2-bit out; OFM_DIM 18: partial tiles in x and y
    (3, 8, 19, 16, 8, 4, 2, 1, 1, 12, 1, 4, 15, -8),        # ap_int<1> lanes (0 / -1), 15 thresholds -> 4-bit two's complement
    (5, 24, 22, 12, 8, 4, 3, 2, 0, 16, 1, 8, 0, 0),         # 2-bit lanes, 24 channels, byte containers out
    (3, 40, 21, 6, 8, 3, 4, 2, 1, 14, 1, 4, 15, -8),        # ap_int<2>, 40 channels; 6 output channels with 4-bit lanes (3 bytes)
    (7, 136, 24, 20, 8, 4, 4, 4, 0, 24, 1, 16, 0, 0),       # 4-bit lanes, 136 channels: three 64-channel chunks, the last partial
    (1, 4, 37, 32, 4, 8, 8, 4, 1, 32, 1, 32, 0, 0),         # 1x1, ap_int<4> lanes, 2-byte pixels; 3 x 3 tiles, partial
    (11, 3, 28, 16, 3, 4, 4, 8, 0, 16, 1, 2, 3, 0),         # K = 11, an RGB-like 3-channel first layer, 2-bit out
    (3, 4, 33, 64, 4, 8, 4, 8, 1, 10, 1, 8, 255, -128),     # 255 thresholds, ActVal -128, 10-bit accumulator
    (3, 8, 18, 70, 8, 7, 3, 8, 0, 20, 0, 16, 1, 0),         # 70 output channels: two workgroup rows, unsigned accumulator
    (5, 16, 17, 24, 8, 8, 2, 2, 0, 8, 1, 2, 3, -2),         # 8-bit wrapping accumulator, 2-bit lanes in and out
    (2, 64, 20, 32, 8, 8, 4, 2, 0, 16, 1, 4, 7, 0),         # K = 2: part of the next chunk is staged after the taps
    (7, 24, 22, 128, 8, 8, 2, 4, 1, 18, 1, 32, 0, 0),       # 4-bit signed lanes, 128 channels out
    (3, 200, 18, 16, 8, 4, 4, 1, 0, 16, 1, 2, 3, 0),        # binary lanes, 200 channels: 25-byte pixels, four chunks
]


def _desc(case):
    from simple_image_compression_network_amd.convlayer import ConvLayerDesc
    K, C, D, O, SIMD, PE, WB, IB, INS, AB, AS, OB, NTH, AV = case
    return ConvLayerDesc(K=K, IFM_CH=C, IFM_DIM=D, OFM_CH=O, SIMD=SIMD, PE=PE, W_BIT=WB, IN_SIGNED=bool(INS), OUT_BIT=OB, IN_BIT=IB)


def _act(case, thr):
    from simple_image_compression_network_amd.convlayer import PassThroughActivation, ThresholdsActivation
    AB, AS, NTH, AV = case[9], case[10], case[12], case[13]
    return ThresholdsActivation(thr, AB, bool(AS), AV) if NTH else PassThroughActivation(AB, bool(AS))


def _odesc(d, act):
    """the oracle's view of a layer (any object with the sicn_convlayer_desc fields)"""
    th = hasattr(act, "m_thresholds")
    return SimpleNamespace(K=d.K, IFM_CH=d.IFM_CH, IFM_DIM=d.IFM_DIM, OFM_CH=d.OFM_CH, OFM_DIM=d.OFM_DIM, SIMD=d.SIMD, PE=d.PE,
                           IN_BIT=d.IN_BIT, IN_SIGNED=int(d.IN_SIGNED), W_BIT=d.W_BIT, W_TILES=d.W_TILES, ACC_BIT=act.ACC_BIT,
                           ACC_SIGNED=int(act.ACC_SIGNED), OUT_BIT=d.OUT_BIT, activation=int(th),
                           NUM_TH=act.m_thresholds.shape[2] if th else 0, ACT_VAL=act.ACT_VAL if th else 0)


def _unpack(out, d):
    """output tensor -> lanes (low OUT_BIT bits), int64 [reps][OD][OD][O]"""
    o = out.cpu().numpy()
    if d.OUT_BIT < 8:
        return sicn_ref.unpack_stream_lanes(o, d.OUT_BIT, d.OFM_CH).astype(np.int64)
    return o.astype(np.int64) & ((1 << d.OUT_BIT) - 1)


def test_kernel_for_names_the_mfma_kernel_for_sub_byte_and_any_channel_layers():
    """sicn_convlayer_kernel_for (pure host): every packed-stream layer and every byte-lane layer with 3, 4 or 8 channels goes to the MFMA
    kernel k_convlayer_patch, byte lanes with IFM_CH % 16 == 0 and OUT_BIT >= 8 stay on k_convlayer_mfma; a descriptor
    sicn_convlayer_validate rejects gets NULL."""
    from simple_image_compression_network_amd import _lib
    from simple_image_compression_network_amd.convlayer import ConvLayerDesc, PassThroughActivation, ThresholdsActivation, kernel_for
    L = _lib.lib()
    descs = []
    for (K, C, D, O, SIMD, PE, WB, IB, INS, AB, AS, OB, NTH, AV) in PACKED_CASES + GRID:
        descs.append(_odesc(ConvLayerDesc(K=K, IFM_CH=C, IFM_DIM=D, OFM_CH=O, SIMD=SIMD, PE=PE, W_BIT=WB, IN_SIGNED=bool(INS), OUT_BIT=OB,
                                          IN_BIT=IB),
                            ThresholdsActivation(np.zeros((PE, O // PE, NTH), np.int32), AB, bool(AS), AV) if NTH
                            else PassThroughActivation(AB, bool(AS))))
    byte_c16 = []                                                            # byte lanes, containers out, C % 16 == 0: k_convlayer_mfma
    for (K, C, D, O, SIMD, PE, WB, INS, AB, AS, OB, NTH, AV) in CASES:
        (byte_c16 if C % 16 == 0 and OB >= 8 else descs).append(SimpleNamespace(K=K, IFM_CH=C, IFM_DIM=D, OFM_CH=O, OFM_DIM=D - K + 1, SIMD=SIMD, PE=PE, IN_BIT=8, IN_SIGNED=INS,
                                     W_BIT=WB, W_TILES=(O // PE) * (K * K * C // SIMD), ACC_BIT=AB, ACC_SIGNED=AS, OUT_BIT=OB,
                                     activation=int(NTH > 0), NUM_TH=NTH, ACT_VAL=AV))
    assert {3, 4, 8} <= {d.IFM_CH for d in descs if d.IN_BIT == 8}
    for d in descs:
        c = _lib.CConvLayerDesc(**{n: int(getattr(d, n)) for n, _ in _lib.CConvLayerDesc._fields_})
        assert L.sicn_convlayer_kernel_for(ctypes.byref(c)) == MFMA.encode(), d
    assert byte_c16
    for d in byte_c16:
        c = _lib.CConvLayerDesc(**{n: int(getattr(d, n)) for n, _ in _lib.CConvLayerDesc._fields_})
        assert L.sicn_convlayer_kernel_for(ctypes.byref(c)) == b"k_convlayer_mfma", d
    assert kernel_for(ConvLayerDesc(K=3, IFM_CH=3, IFM_DIM=130, OFM_CH=64, SIMD=3, PE=8, OUT_BIT=2),
                      ThresholdsActivation(np.zeros((8, 8, 3), np.int32))) == MFMA
    good = ConvLayerDesc(K=3, IFM_CH=4, IFM_DIM=9, OFM_CH=6, SIMD=2, PE=3).to_c(PassThroughActivation(16, True))
    assert L.sicn_convlayer_kernel_for(ctypes.byref(good)) == MFMA.encode()
    for field, val in (("K", 12), ("IN_BIT", 3), ("OUT_BIT", 2), ("OFM_DIM", 9), ("NUM_TH", 2)):
        bad = ConvLayerDesc(K=3, IFM_CH=4, IFM_DIM=9, OFM_CH=6, SIMD=2, PE=3).to_c(PassThroughActivation(16, True))
        setattr(bad, field, val)
        assert L.sicn_convlayer_kernel_for(ctypes.byref(bad)) is None, field
    assert L.sicn_convlayer_kernel_for(None) is None
    assert kernel_for(ConvLayerDesc(K=3, IFM_CH=4, IFM_DIM=9, OFM_CH=6, SIMD=2, PE=3, IN_BIT=1), PassThroughActivation(16, True)) is None
    assert L.sicn_version() >= 4


def _make(case, rng, reps=2):
    K, C, D, O, SIMD, PE, WB, IB, INS, AB, AS, OB, NTH, AV = case
    nf = O // PE
    w = rng.integers(-(1 << (WB - 1)), 1 << (WB - 1), (O, K * K * C)).astype(np.int8)
    words = sicn_ref.pack_finn_tiles_generic(w, SIMD, PE, WB)
    lanes = rng.integers(0, 1 << IB, (reps, D, D, C)).astype(np.uint8)     # distinct images
    thr = None
    if NTH:
        # thresholds spread over the accumulator's typical range, so that the counts vary
        span = int(min(1 << (AB - 1), 3 * (1 << (WB - 1)) * (1 << IB) * np.sqrt(K * K * C) + 8))
        thr = np.sort(rng.integers(-span if AS else 0, span, (PE, nf, NTH)), axis=2).astype(np.int32)
    return w, words, lanes, thr


def _run_case(case, seed):
    import torch
    from simple_image_compression_network_amd.api import FixedPointWeights
    from simple_image_compression_network_amd.convlayer import ConvLayer, kernel_for
    rng = np.random.default_rng(seed)
    d = _desc(case)
    w, words, lanes, thr = _make(case, rng)
    act = _act(case, thr)
    assert kernel_for(d, act) == MFMA
    layer = ConvLayer(d, FixedPointWeights(d.SIMD, d.W_BIT, d.PE, d.W_TILES, words), act)
    assert layer.kernel == MFMA
    xin = torch.from_numpy(sicn_ref.pack_stream_lanes(lanes, d.IN_BIT)).cuda()
    auto = layer(xin, None, 2)
    direct = layer(xin, None, 2, kernel=1)
    torch.cuda.synchronize()
    layer.close()
    assert torch.equal(auto, direct)
    got = _unpack(auto, d)
    for i in range(2):
        ref = c_oracle.convlayer_dataflow(_odesc(d, act), words, thr, lanes[i], use_fsm=False)
        assert np.array_equal(got[i], ref.astype(np.int64)), f"image {i}"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRID)
def test_gpu_mfma_kernel_matches_direct_kernel_and_dataflow(case):
    got = _run_case(case, GRID.index(case))
    assert len(np.unique(got)) > 1                                           # the comparison is not between constant planes


@pytest.mark.gpu
@pytest.mark.parametrize("case", PACKED_CASES)
def test_gpu_mfma_kernel_serves_the_packed_cases(case):
    _run_case(case, 100 + PACKED_CASES.index(case))


@pytest.mark.gpu
def test_gpu_three_thresholded_layers_chain_on_the_mfma_kernel():
    """8-bit RGB-like lanes (3 channels) -> 3 thresholds -> 2-bit lanes -> 3 thresholds -> 2-bit lanes -> 15 thresholds -> 4-bit lanes.
    Each output buffer is handed to the next layer untouched; every layer runs on the MFMA kernel and equals the restated dataflow fed
    with the previous layer's GPU output."""
    import torch
    from simple_image_compression_network_amd.api import FixedPointWeights
    from simple_image_compression_network_amd.convlayer import ConvLayer, ConvLayerDesc, ThresholdsActivation
    rng = np.random.default_rng(31)
    D = 36
    specs = [  # (C, O, SIMD, PE, W_BIT, IN_BIT, OUT_BIT, NUM_TH, threshold span)
        (3, 16, 3, 4, 4, 8, 2, 3, 2000),
        (16, 24, 8, 4, 2, 2, 2, 3, 40),
        (24, 8, 8, 2, 2, 2, 4, 15, 50),
    ]
    x = rng.integers(0, 256, (2, D, D, 3), dtype=np.uint8)
    buf = torch.from_numpy(x).cuda()
    lanes, dim = x, D
    for (C, O, SIMD, PE, WB, IB, OB, NTH, span) in specs:
        d = ConvLayerDesc(K=3, IFM_CH=C, IFM_DIM=dim, OFM_CH=O, SIMD=SIMD, PE=PE, W_BIT=WB, IN_SIGNED=False, OUT_BIT=OB, IN_BIT=IB)
        w = rng.integers(-(1 << (WB - 1)), 1 << (WB - 1), (O, 9 * C)).astype(np.int8)
        words = sicn_ref.pack_finn_tiles_generic(w, SIMD, PE, WB)
        thr = np.sort(rng.integers(-span, span, (PE, O // PE, NTH)), axis=2).astype(np.int32)
        act = ThresholdsActivation(thr, 16, True, 0)
        layer = ConvLayer(d, FixedPointWeights(SIMD, WB, PE, d.W_TILES, words), act)
        assert layer.kernel == MFMA
        out = layer(buf, None, 2)                                            # the previous layer's buffer, as it is
        torch.cuda.synchronize()
        layer.close()
        assert tuple(out.shape) == (2, d.OFM_DIM, d.OFM_DIM, O * OB // 8)
        got = sicn_ref.unpack_stream_lanes(out.cpu().numpy(), OB, O)
        for i in range(2):
            ref = c_oracle.convlayer_dataflow(_odesc(d, act), words, thr, lanes[i], use_fsm=True)
            assert np.array_equal(got[i], ref)
            assert np.array_equal(out[i].cpu().numpy(), sicn_ref.pack_stream_lanes(ref, OB))
        assert len(np.unique(got)) > 1
        buf, lanes, dim = out, got.astype(np.uint8), d.OFM_DIM


@pytest.mark.gpu
def test_gpu_mfma_kernel_matches_direct_kernel_on_a_large_layer():
    """3x3x256 -> 256, 2-bit lanes in and out, 4 x 66^2 (too large for the oracle): AUTO bytes == DIRECT bytes."""
    import torch
    from simple_image_compression_network_amd.api import FixedPointWeights
    from simple_image_compression_network_amd.convlayer import ConvLayer, ConvLayerDesc, ThresholdsActivation
    rng = np.random.default_rng(256)
    K, C, D, O = 3, 256, 66, 256
    d = ConvLayerDesc(K=K, IFM_CH=C, IFM_DIM=D, OFM_CH=O, SIMD=16, PE=16, W_BIT=2, IN_SIGNED=False, OUT_BIT=2, IN_BIT=2)
    w = rng.integers(-1, 2, (O, K * K * C)).astype(np.int8)                  # zero-mean: the accumulators spread around 0 (sd ~ 75)
    thr = np.sort(rng.integers(-120, 120, (16, O // 16, 3)), axis=2).astype(np.int32)
    act = ThresholdsActivation(thr, 16, True, 0)
    layer = ConvLayer(d, FixedPointWeights(16, 2, 16, d.W_TILES, sicn_ref.pack_finn_tiles_generic(w, 16, 16, 2)), act)
    assert layer.kernel == MFMA
    x = torch.from_numpy(sicn_ref.pack_stream_lanes(rng.integers(0, 4, (4, D, D, C)).astype(np.uint8), 2)).cuda()
    auto = layer(x, None, 4)
    direct = layer(x, None, 4, kernel=1)
    torch.cuda.synchronize()
    layer.close()
    assert torch.equal(auto, direct)
    assert len(np.unique(sicn_ref.unpack_stream_lanes(auto.cpu().numpy(), 2, O))) == 4
