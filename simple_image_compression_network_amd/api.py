"""Host-side mirror of the reference's operator interface for the transform path.

Reference surface (conv_nonsquare_top.cpp):
    conv2d<...>(weights, bias, in, out, numReps)            :198-280
    deconv522<...>(weights, bias, in, out, numReps)         :71-195
    conv2d_layer0(in, out, numReps)                         :282-286
    deconv2d_layer4(in, out, numReps)                       :288-291
    eight_layers_net(in, out, numReps)                      :295-357
    FixedPointWeights<SIMD, ap_int<4>, PE, TILES>           weights.hpp:110-150

Same names, argument order and meaning; the `hls::stream<ap_uint<C*8>>` arguments become CUDA/HIP
`torch.uint8` tensors of shape [numReps][H][W][C] (byte-identical to the stream), and
`numReps` is a true batch (the reference is only well defined at numReps == 1).
Everything here is plumbing over the C ABI of include/sicn.h: torch supplies device memory and
streams, nothing else.  No CPU path exists: tensors must live on the GPU.
"""
from __future__ import annotations

import ctypes
from dataclasses import replace
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .config import CLayerDesc, LayerDesc, REFERENCE_DESCS, eight_layer_descs

__all__ = ["FixedPointWeights", "DeviceWeights", "conv2d", "deconv522", "conv2d_layer0", "deconv2d_layer4",
           "eight_layers_net", "EightLayersNet", "RaggedNet", "RaggedCrop", "RaggedCut", "RaggedRoi", "MovingRoi", "roi_plan", "load_param_weights", "PARAM", "GDN"]

_DATA = Path(__file__).resolve().parent / "data" / "param_weights.npz"


class FixedPointWeights:
    """`FixedPointWeights<SIMD, ap_int<W_BIT>, PE, TILES>` (weights.hpp:110-150): `m_weights[PE][TILES]`
    words, element s of a word = sign-extended nibble in bits [4s, 4s+4)."""

    def __init__(self, SIMD: int, W_BIT: int, PE: int, TILES: int, m_weights):
        if not 2 <= W_BIT <= 8 or SIMD * W_BIT > 64:
            raise ValueError("W_BIT must be 2..8 and SIMD*W_BIT <= 64 (the net itself uses ap_int<4> tiles, ap_int<8> biases)")
        self.SIMD, self.W_BIT, self.PE, self.TILES = SIMD, W_BIT, PE, TILES
        self.m_weights = np.ascontiguousarray(m_weights, dtype=np.uint64).reshape(PE, TILES)

    def bias_values(self) -> np.ndarray:
        """`bias.weights(j)[0][0]` for every j (conv_nonsquare_top.cpp:272) as int8."""
        assert self.SIMD == 1 and self.PE == 1 and self.W_BIT == 8
        return self.m_weights.reshape(-1).astype(np.uint8).view(np.int8)


def _stream_ptr(stream) -> ctypes.c_void_p:
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(getattr(stream, "cuda_stream", stream))


def _check_tensor(t, shape, what):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise TypeError(f"{what}: need a contiguous torch.uint8 CUDA tensor (no CPU path exists)")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: shape {tuple(t.shape)} != {tuple(shape)}")


class DeviceWeights(_lib.Handle):
    """One layer's weights + bias uploaded through `sicn_weights_from_finn_tiles`."""
    _free = "sicn_weights_free"

    def __init__(self, desc: LayerDesc, weights: FixedPointWeights, bias):
        L = _lib.lib()
        if (weights.SIMD, weights.PE, weights.TILES) != (desc.SIMD, desc.PE, desc.W_TILES):
            raise ValueError("FixedPointWeights fold does not match the layer descriptor")
        b = bias.bias_values() if isinstance(bias, FixedPointWeights) else np.ascontiguousarray(bias, np.int8)
        if b.shape != (desc.OFM_CH,):
            raise ValueError("bias must have OFM_CH entries")
        self._h = ctypes.c_void_p()
        cd = desc.to_c()
        _lib.check(L.sicn_weights_from_finn_tiles(ctypes.byref(cd), weights.m_weights.ctypes.data_as(ctypes.c_void_p),
                                                  8, b.ctypes.data_as(ctypes.c_void_p), ctypes.byref(self._h)),
                   "sicn_weights_from_finn_tiles")
        self.key = (desc.IFM_CH, desc.OFM_CH, desc.transposed)

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h


class GDN(_lib.Handle):
    """Fixed-point GDN (inverse=False) / IGDN (inverse=True) activation, include/sicn_gdn.h.  EXTENSION BEYOND THE
    REFERENCE (it has no GDN, activations.hpp:127-224); replaces a layer's sign-bit ReLU (conv_nonsquare_top.cpp:273-275).
    beta: uint32 [C] in [1, 65535]; gamma: uint8 [C][C] in [0, 127]; shift in [1, 24]."""
    _free = "sicn_gdn_free"

    def __init__(self, beta, gamma, inverse: bool = False, shift: int = 12):
        beta = np.ascontiguousarray(beta, dtype=np.uint32)
        gamma = np.ascontiguousarray(gamma, dtype=np.uint8)
        c = int(beta.shape[0])
        if gamma.shape != (c, c):
            raise ValueError("gamma must be [C][C]")
        self.channels, self.inverse, self.shift = c, bool(inverse), int(shift)
        self._h = ctypes.c_void_p()
        _lib.check(_lib.lib().sicn_gdn_create(c, int(self.inverse), self.shift, beta.ctypes.data_as(ctypes.c_void_p),
                                              gamma.ctypes.data_as(ctypes.c_void_p), ctypes.byref(self._h)), "sicn_gdn_create")

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def apply_(self, lanes, stream=None):
        """In place over a contiguous CUDA uint8 tensor [...][C] of pre-activation lanes."""
        import torch
        if not (isinstance(lanes, torch.Tensor) and lanes.is_cuda and lanes.dtype == torch.uint8 and lanes.is_contiguous()
                and lanes.shape[-1] == self.channels):
            raise TypeError("lanes: need a contiguous CUDA uint8 tensor [...][C]")
        _lib.check(_lib.lib().sicn_gdn_apply(self._h, ctypes.c_void_p(lanes.data_ptr()), lanes.numel() // self.channels,
                                             _stream_ptr(stream)), "sicn_gdn_apply")
        return lanes


def _as_device(desc, weights, bias) -> DeviceWeights:
    return weights if isinstance(weights, DeviceWeights) else DeviceWeights(desc, weights, bias)


def _opt_ptr(options):
    """options: None (library defaults), a dict of sicn_options fields, or a _lib.COptions."""
    if options is None:
        return None
    if isinstance(options, dict):
        options = _lib.make_options(**options)
    return ctypes.byref(options)


def _run(fn_name, desc, weights, bias, in_, out, numReps, stream, options=None, gdn=None):
    import torch
    L = _lib.lib()
    desc.validate()
    dw = _as_device(desc, weights, bias)
    _check_tensor(in_, (numReps,) + desc.in_shape, "in")
    if out is None:
        out = torch.empty((numReps,) + desc.out_shape, dtype=torch.uint8, device=in_.device)
    _check_tensor(out, (numReps,) + desc.out_shape, "out")
    cd = desc.to_c()
    if gdn is not None:
        _lib.check(getattr(L, fn_name + "_gdn")(ctypes.byref(cd), dw.handle, gdn.handle, ctypes.c_void_p(in_.data_ptr()),
                                                ctypes.c_void_p(out.data_ptr()), numReps, _opt_ptr(options),
                                                _stream_ptr(stream)), fn_name + "_gdn")
        return out
    _lib.check(getattr(L, fn_name + "_opt")(ctypes.byref(cd), dw.handle, ctypes.c_void_p(in_.data_ptr()),
                                            ctypes.c_void_p(out.data_ptr()), numReps, _opt_ptr(options),
                                            _stream_ptr(stream)), fn_name)
    return out


def conv2d(desc: LayerDesc, weights, bias, in_, out=None, numReps: int = 1, stream=None, options=None, gdn=None):
    """`conv2d<...>(weights, bias, in, out, numReps)` — conv_nonsquare_top.cpp:198-280.
    `options`: sicn_options fields as a dict (kernel-selection knobs for tests / experiments).
    `gdn`: a GDN object to apply in place of the ReLU (extension beyond the reference)."""
    return _run("sicn_conv2d", desc, weights, bias, in_, out, numReps, stream, options, gdn)


def deconv522(desc: LayerDesc, weights, bias, in_, out=None, numReps: int = 1, stream=None, options=None, gdn=None):
    """`deconv522<...>(weights, bias, in, out, numReps)` — conv_nonsquare_top.cpp:71-195."""
    return _run("sicn_deconv522", desc, weights, bias, in_, out, numReps, stream, options, gdn)


# ---- the PARAM:: tables (memdata_nonsquare.h) -------------------------------------------------
def load_param_weights(path=None):
    """[(FixedPointWeights weights_layerN, FixedPointWeights bias_layerN)] * 8 — `namespace PARAM`."""
    z = np.load(path or _DATA)
    out = []
    for n in range(8):
        simd, wbit, pe, tiles = (int(v) for v in z[f"w{n}_meta"])
        b = z[f"b{n}"]
        out.append((FixedPointWeights(simd, wbit, pe, tiles, z[f"w{n}_words"]),
                    FixedPointWeights(1, 8, 1, b.size, b.view(np.uint8).astype(np.uint64))))
    return out


class _Param:
    """Lazy `PARAM::weights_layerN` / `PARAM::bias_layerN`."""
    _tables = None

    def __getattr__(self, name):
        if _Param._tables is None:
            _Param._tables = load_param_weights()
        kind, _, n = name.partition("_layer")
        if kind in ("weights", "bias") and n.isdigit() and int(n) < 8:
            return _Param._tables[int(n)][0 if kind == "weights" else 1]
        raise AttributeError(name)


PARAM = _Param()


class EightLayersNet(_lib.Handle):
    """`eight_layers_net` (conv_nonsquare_top.cpp:295-357) for one image size: descriptors, device
    weights, the chain handle and its ping-pong workspace.  `forward` enqueues the 8 layers on the
    current stream and returns (reconstruction, latent)."""
    _free = "sicn_net_free"

    def __init__(self, width: int = 768, height: int = 512, params=None, device=None,
                 descs: Optional[Sequence[LayerDesc]] = None, shared_weights: Optional[Sequence[DeviceWeights]] = None,
                 options=None, gdn: Optional[Sequence[Optional["GDN"]]] = None):
        import torch
        L = _lib.lib()
        self.descs: List[LayerDesc] = list(descs) if descs is not None else eight_layer_descs(width, height)
        self.device = torch.device(device if device is not None else "cuda")
        if shared_weights is not None:
            self.weights = list(shared_weights)
        else:
            params = params if params is not None else load_param_weights()
            with torch.cuda.device(self.device):
                self.weights = [DeviceWeights(d, w, b) for d, (w, b) in zip(self.descs, params)]
        n = len(self.descs)
        cdescs = (CLayerDesc * n)(*[d.to_c() for d in self.descs])
        handles = (ctypes.c_void_p * n)(*[w.handle for w in self.weights])
        self._h = ctypes.c_void_p()
        self.gdn = list(gdn) if gdn is not None else None      # keeps the activations alive
        if self.gdn is not None:
            if len(self.gdn) != n:
                raise ValueError("gdn must have one entry (or None) per layer")
            ghandles = (ctypes.c_void_p * n)(*[(g.handle if g is not None else None) for g in self.gdn])
            _lib.check(L.sicn_net_create_gdn(cdescs, handles, ghandles, n, _opt_ptr(options), ctypes.byref(self._h)),
                       "sicn_net_create_gdn")
        else:
            _lib.check(L.sicn_net_create_opt(cdescs, handles, n, _opt_ptr(options), ctypes.byref(self._h)), "sicn_net_create_opt")
        self._ws = None
        self._ws_bytes = {}

    def workspace(self, n_images: int):
        import torch
        # the size the library asks for per batch size, cached; the buffer never shrinks.  No initialisation is needed
        # (sicn.h: sicn_net_forward zeroes the tile-deal words behind the ping-pong buffers itself).
        nbytes = self._ws_bytes.get(n_images)
        if nbytes is None:
            nbytes = self._ws_bytes[n_images] = max(int(_lib.lib().sicn_net_workspace_bytes(self._h, n_images)), 256)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def forward(self, in_, out=None, latent=None, numReps: Optional[int] = None, want_latent: bool = True, stream=None):
        import torch
        L = _lib.lib()
        n = in_.shape[0] if numReps is None else numReps
        _check_tensor(in_, (n,) + self.descs[0].in_shape, "in")
        if out is None:
            out = torch.empty((n,) + self.descs[-1].out_shape, dtype=torch.uint8, device=in_.device)
        _check_tensor(out, (n,) + self.descs[-1].out_shape, "out")
        lat_ptr = ctypes.c_void_p(0)
        if want_latent and len(self.descs) > 3:
            if latent is None:
                latent = torch.empty((n,) + self.descs[3].out_shape, dtype=torch.uint8, device=in_.device)
            _check_tensor(latent, (n,) + self.descs[3].out_shape, "latent")
            lat_ptr = ctypes.c_void_p(latent.data_ptr())
        ws = self.workspace(n)
        _lib.check(L.sicn_eight_layers_net(self._h, ctypes.c_void_p(in_.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                           lat_ptr, n, ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream_ptr(stream)),
                   "sicn_eight_layers_net")
        return out, latent

    def capture(self, in_, out, latent=None):
        """The whole forward pass as ONE replayable hipGraph (the launch functions neither allocate nor
        synchronise, sicn.h): for small images the 8 launches cost more host time than device time.
        Returns a torch.cuda.CUDAGraph; `.replay()` recomputes `out` / `latent` from the current contents
        of `in_` (same tensors).  Keep other frees (net objects, tensors) out of the capture window."""
        import gc
        import torch
        self.forward(in_, out, latent, want_latent=latent is not None)      # warm-up: module load, workspace
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=in_.device)
        gc.collect()
        gc_was = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    self.forward(in_, out, latent, want_latent=latent is not None)
        finally:
            if gc_was:
                gc.enable()
        return graph

    def analysis(self, in_, latent=None, stream=None):
        """Encoder half: layers 0..3, image batch -> latent (conv_3_out, conv_nonsquare_top.cpp:322-325)."""
        return self.run_layers(0, 3, in_, out=latent, stream=stream)[0]

    def synthesis(self, latent, out=None, stream=None):
        """Decoder half: layers 4..7, latent -> reconstruction."""
        return self.run_layers(4, len(self.descs) - 1, latent, out=out, stream=stream)[0]

    def run_layers(self, first: int, last: int, in_, tap_layer: int = -1, stream=None, out=None):
        """Layers [first, last] of the chain (sicn_net_forward); returns (out, tap or None)."""
        import torch
        L = _lib.lib()
        n = in_.shape[0]
        _check_tensor(in_, (n,) + self.descs[first].in_shape, "in")
        if out is None:
            out = torch.empty((n,) + self.descs[last].out_shape, dtype=torch.uint8, device=in_.device)
        _check_tensor(out, (n,) + self.descs[last].out_shape, "out")
        tap = None
        tap_ptr = ctypes.c_void_p(0)
        if tap_layer >= 0:
            tap = torch.empty((n,) + self.descs[tap_layer].out_shape, dtype=torch.uint8, device=in_.device)
            tap_ptr = ctypes.c_void_p(tap.data_ptr())
        ws = self.workspace(n)
        _lib.check(L.sicn_net_forward(self._h, first, last, ctypes.c_void_p(in_.data_ptr()),
                                      ctypes.c_void_p(out.data_ptr()), tap_layer, tap_ptr, n,
                                      ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream_ptr(stream)), "sicn_net_forward")
        return out, tap

    # measurement aids (sicn_net_profile / sicn_net_layer_ms)
    def profile(self, enable: bool = True) -> None:
        _lib.check(_lib.lib().sicn_net_profile(self._h, int(enable)), "sicn_net_profile")

    def layer_ms(self, reset: bool = True):
        n = len(self.descs)
        ms = (ctypes.c_float * n)()
        cnt = (ctypes.c_int * n)()
        _lib.check(_lib.lib().sicn_net_layer_ms(self._h, int(reset), ms, cnt), "sicn_net_layer_ms")
        return list(ms), list(cnt)


class RaggedCut(_lib.Handle):
    """A rectangle out of every image of a ragged tensor, ONE launch for the batch (sicn_ragged_cut_*, include/sicn_ragged_window.h).
    src_shapes: [(h, w)] per image; rects: [(x0, y0, w, h)] per image, inside its source; both tensors are flat uint8 CUDA tensors, the
    images' [h][w][channels] arrays back to back — or, for the source, at `src_offsets` (bytes, one per image).  RaggedCrop (below) is
    the case x0 = y0 = 0."""
    _free = "sicn_ragged_cut_free"

    def __init__(self, src_shapes, rects, channels: int, src_offsets=None, device=None):
        import torch
        L = _lib.lib()
        self.src_shapes = [(int(h), int(w)) for h, w in src_shapes]
        self.rects = [tuple(int(v) for v in r) for r in rects]
        self.channels = int(channels)
        n = len(self.src_shapes)
        if len(self.rects) != n or any(len(r) != 4 for r in self.rects):
            raise ValueError("rects: one (x0, y0, w, h) per source shape")
        if src_offsets is not None and len(src_offsets) != n:
            raise ValueError("src_offsets: one per source shape")
        for (h, w), (x0, y0, rw, rh) in zip(self.src_shapes, self.rects):
            if rw < 1 or rh < 1 or x0 < 0 or y0 < 0 or x0 + rw > w or y0 + rh > h:
                raise ValueError(f"rectangle {(x0, y0, rw, rh)} is empty or outside its {w} x {h} source")
        i32 = ctypes.c_int32 * max(n, 1)
        sw, sh = i32(*[w for _, w in self.src_shapes]), i32(*[h for h, _ in self.src_shapes])
        crects = (_lib.RaggedRect * max(n, 1))(*[_lib.RaggedRect(*r) for r in self.rects])
        offs = None if src_offsets is None else (ctypes.c_uint64 * max(n, 1))(*[int(o) for o in src_offsets])
        self.dst_shapes = [(rh, rw) for _, _, rw, rh in self.rects]
        self._src_off, self._dst_off = [], []
        q = (ctypes.c_int64 * 4)()
        for i in range(n):
            _lib.check(L.sicn_ragged_cut_layout(sw, sh, crects, self.channels, offs, n, i, q), "sicn_ragged_cut_layout")
            self._src_off.append(int(q[0]))
            self._dst_off.append(int(q[1]))
        self.src_bytes, self.dst_bytes = int(q[2]), int(q[3])      # src_bytes: the furthest byte a source image reaches
        self.device = torch.device(device if device is not None else "cuda")
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.sicn_ragged_cut_create(sw, sh, crects, self.channels, offs, n, ctypes.byref(self._h)), "sicn_ragged_cut_create")

    def views(self, dst):
        """Per-image [h][w][channels] views of a destination tensor (no copy)."""
        _check_tensor(dst, (self.dst_bytes,), "dst")
        c = self.channels
        return [dst[o:o + h * w * c].view(h, w, c) for o, (h, w) in zip(self._dst_off, self.dst_shapes)]

    def run(self, src, dst=None, stream=None):
        """src (flat, at least src_bytes long) -> dst (ragged, the rectangles' shapes; allocated when None).  Enqueue only."""
        import torch
        if not (src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 1 and src.numel() >= self.src_bytes):
            raise TypeError(f"src must be a flat contiguous CUDA uint8 tensor of at least {self.src_bytes} bytes")
        if dst is None:
            dst = torch.empty(self.dst_bytes, dtype=torch.uint8, device=src.device)
        _check_tensor(dst, (self.dst_bytes,), "dst")
        _lib.check(_lib.lib().sicn_ragged_cut_run(self._h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
                                                  _stream_ptr(stream)), "sicn_ragged_cut_run")
        return dst


class RaggedCrop(RaggedCut):
    """Every image of a ragged tensor cut to its top-left corner, ONE launch for the batch: RaggedCut with the rectangles
    (0, 0, w, h) and both tensors back to back (sicn_ragged_crop_* of include/sicn_ragged_hyper.h are that cut too).
    src_shapes / dst_shapes: [(h, w)] per image, dst no larger than src.  What the chain rule rounds up is cut back with it: h_s(z)
    to the latent's shape, a reconstruction to the image's size."""

    def __init__(self, src_shapes, dst_shapes, channels: int, device=None):
        src_shapes, dst_shapes = list(src_shapes), list(dst_shapes)
        if len(dst_shapes) != len(src_shapes):
            raise ValueError("dst_shapes: one (h, w) per source shape")
        super().__init__(src_shapes, [(0, 0, w, h) for h, w in dst_shapes], channels, device=device)

    def views(self, packed, which: str = "dst"):
        """Per-image [h][w][channels] views of a destination (which="dst") or source (which="src") tensor (no copy)."""
        if which == "dst":
            return super().views(packed)
        _check_tensor(packed, (self.src_bytes,), which)
        c = self.channels
        return [packed[o:o + h * w * c].view(h, w, c) for o, (h, w) in zip(self._src_off, self.src_shapes)]

    def run(self, src, dst=None, stream=None):
        """src (ragged, source shapes, exactly src_bytes long) -> dst (ragged, destination shapes; allocated when None).  Enqueue only."""
        _check_tensor(src, (self.src_bytes,), "src")
        return super().run(src, dst, stream)


def _raise_on_status(status, what):
    """Raises for a batch's decoder verdicts (one word per image) unless all are 0: SICN_EBADMSG (-74) where nothing but the
    checksum of a whole latent (bit 7) failed, SICN_EINVAL (-22) otherwise.  A window decode never sets bit 7."""
    if any(status):
        raise _lib.SicnError(-22 if any(v & ~128 for v in status) else -74, f"{what} status {status}")


def roi_plan(size, rect, n_up_layers: int = 4):
    """What the pixel rectangle `rect` = (x0, y0, w, h) of an image of `size` = (width, height) needs of its latent
    (sicn_ragged_roi_plan): a dict with the latent window `c0, r0, cw, rh`, the rectangle's corner `x, y` inside the window's
    reconstruction, and the margins.  ValueError for a rectangle that is empty or reaches outside the image."""
    w, h = int(size[0]), int(size[1])
    if len(rect) != 4:
        raise ValueError("rect: (x0, y0, w, h)")
    r = _lib.RaggedRect(*[int(v) for v in rect])
    s = 1 << n_up_layers
    out = _lib.RaggedRoiPlan()
    rc = _lib.lib().sicn_ragged_roi_plan(n_up_layers, w, h, (w + s - 1) // s, (h + s - 1) // s, ctypes.byref(r), ctypes.byref(out))
    if rc == -22:
        raise ValueError(f"rectangle {tuple(rect)} is empty or reaches outside the {w} x {h} image")
    _lib.check(rc, "sicn_ragged_roi_plan")
    return {k: int(getattr(out, k)) for k, _ in _lib.RaggedRoiPlan._fields_}


def _refuse_planar(net, what):
    """The ROI decodes cut their pixels from interleaved rows (k_ragged_cut): a net with planar pixels is refused before any launch."""
    if getattr(net, "planar_in", False) or getattr(net, "planar_out", False):
        raise ValueError(f"{what}: the ROI decodes have no planar form; make the net with rgb_layout='interleaved'")


def _roi_options(net, what, roi_layout, direct):
    """The keywords `roi_layout` and `direct` of an ROI decode -> (layout, direct).  roi_layout None is today's chain: interleaved
    pixels, and a net with planar pixels is refused.  "interleaved" or "planar" name the layout of the ROI pixels whatever the net's
    own layout is — it plays no part in layers 4-7.  direct: layer 7 stores the rectangles itself (include/sicn_ragged_rect.h), no
    reconstruction tensor and no cut launch; None means True for planar, which has no other form, and False for interleaved."""
    if roi_layout is None:
        _refuse_planar(net, what)
        roi_layout = "interleaved"
    elif roi_layout not in _lib.RAGGED_PIXELS:
        raise ValueError(f"roi_layout: 'interleaved' or 'planar', not {roi_layout!r}")
    if direct is None:
        direct = roi_layout == "planar"
    if roi_layout == "planar" and not direct:
        raise ValueError("roi_layout='planar' has no form with a pixel cut: direct must be True (or None)")
    return roi_layout, bool(direct)


def _roi_chain(net, plans, rects, bands, first_rows, roi_layout="interleaved", direct=False):
    """What follows a window decoder in an ROI decode, shared by RaggedRoi and hyperprior.RaggedHyperpriorRoi: (the latent cut, the
    window net, the pixel cut).  bands: per image (the latent rows its band holds, the band's byte offset in the band tensor);
    first_rows: the band row at which the plan's row r0 lies.  The window net runs layers 4 .. on `net`'s weights, descs and GDN
    objects over the sizes (16 cw, 16 rh).  direct: the window net is made with the rectangles (x, y, w, h) inside the windows'
    reconstructions, its last layer writes the ROI pixels in `roi_layout` and there is no pixel cut (None)."""
    lat = net.shapes(3)
    latent_cut = RaggedCut([(rows, w) for (rows, _), (_, w, _) in zip(bands, lat)],
                           [(p["c0"], y0, p["cw"], p["rh"]) for p, y0 in zip(plans, first_rows)], lat[0][2],
                           src_offsets=[off for _, off in bands], device=net.device)
    if direct:
        window_net = RaggedNet([(16 * p["cw"], 16 * p["rh"]) for p in plans], device=net.device, shared_weights=net.weights,
                               descs=net.descs, gdn=net.gdn, out_rects=[(p["x"], p["y"], r[2], r[3]) for p, r in zip(plans, rects)],
                               out_layout=roi_layout)
        return latent_cut, window_net, None
    window_net = RaggedNet([(16 * p["cw"], 16 * p["rh"]) for p in plans], device=net.device, shared_weights=net.weights,
                           descs=net.descs, gdn=net.gdn)
    pixel_cut = RaggedCut([(16 * p["rh"], 16 * p["cw"]) for p in plans], [(p["x"], p["y"], r[2], r[3]) for p, r in zip(plans, rects)],
                          net.shapes(len(net.descs) - 1)[0][2], device=net.device)
    return latent_cut, window_net, pixel_cut


class RaggedRoi:
    """One pixel rectangle of every image of a RaggedNet's batch, decoded from the images' rANS-W containers without the rest of the
    image (include/sicn_ragged_window.h): 2 + 1 + 4 + 1 launches whatever the number of images — the window decoder over the streams
    that hold the latent rows, the cut of the latent columns, layers 4-7 of a second RaggedNet made for the windows' sizes
    (16 cw, 16 rh) on `net`'s weights, the cut of the rectangle.  Same bytes as the full decode, sliced.
    rects: one (x0, y0, w, h) per image, or None for that image whole.  One rectangle per image: two details of one photograph are
    two objects (and, through an archive, two calls).  coder: the RaggedLatentCoder whose slots hold the containers (default: a new
    one from net.latent_coder(stream_symbols)).
    roi_layout, direct: see `_roi_options`.  With `direct`, layer 7 of the window net stores the rectangles itself — [h][w][3] or,
    planar, [3][h][w] per image: seven launches, no reconstruction tensor; `pixel_cut` is None."""

    def __init__(self, net, rects, coder=None, stream_symbols=16384, roi_layout=None, direct=None):
        self.roi_layout, self.direct = _roi_options(net, "RaggedRoi", roi_layout, direct)
        n = len(net.sizes)
        if len(rects) != n:
            raise ValueError(f"rects: one per image, {n}")
        self.net = net
        self.rects = [(0, 0, w, h) if r is None else tuple(int(v) for v in r) for r, (w, h) in zip(rects, net.sizes)]
        self.plans = [roi_plan(size, r) for size, r in zip(net.sizes, self.rects)]        # ValueError before anything is made
        self.coder = coder if coder is not None else net.latent_coder(stream_symbols)
        lat = net.shapes(3)
        if [(h, w) for h, w, _ in lat] != self.coder.shapes or lat[0][2] != self.coder.lat_c:
            raise ValueError("the coder's latent shapes are not the net's")
        self.window = self.coder.window([(p["r0"], p["rh"]) for p in self.plans])
        # a band begins inside a stream: rows from r0 on, `lead` bytes in
        self.latent_cut, self.window_net, self.pixel_cut = _roi_chain(
            net, self.plans, self.rects, [(p["rh"], int(im.band_offset) + int(im.lead)) for p, im in zip(self.plans, self.window.images)],
            [0] * n, self.roi_layout, self.direct)
        self.status = self.window.status

    def decode(self, slots=None, valid=None, stream=None, out=None):
        """The coder's slots (or `slots`, `valid` as in RaggedLatentCoder.decode) -> the ROI pixels, a ragged [h][w][3] tensor
        ([3][h][w] per image with roi_layout="planar").  Enqueue only: eight launches, seven with `direct`.  `self.status` holds the
        window decoder's verdicts."""
        import torch
        dev = self.net.device
        self.band = torch.empty(self.window.band_bytes, dtype=torch.uint8, device=dev)
        self.window.decode(self.band, slots=slots, valid=valid, stream=stream)
        self.latent = self.latent_cut.run(self.band, stream=stream)
        if self.direct:
            return self.window_net.run_layers(4, len(self.net.descs) - 1, self.latent, out=out, stream=stream)[0]
        recon, _ = self.window_net.run_layers(4, len(self.net.descs) - 1, self.latent, stream=stream)
        return self.pixel_cut.run(recon, out, stream=stream)

    def views(self, roi):
        """Per-image [h][w][3] views of what `decode` returned ([3][h][w] with roi_layout="planar")."""
        if self.direct:
            return self.window_net.views(len(self.net.descs) - 1, roi)
        return self.pixel_cut.views(roi)


class _MovingRoiChain(_lib.Handle):
    """What MovingRoi and hyperprior.MovingHyperpriorRoi share: the slots, the library object and its layout, the window net, the
    chain's tensors, the positions and everything of a decode that follows its coder's arguments.  A subclass names its entry
    points in `_abi` (`<_abi>_layout`, `_create`, `_workspace_bytes`, `_decode_async`, `_cut_async`), the struct of its layout in
    `_slot_type` and the number of its layout's totals in `_n_totals` (the first five are the tensors' bytes)."""
    _abi, _slot_type, _n_totals = "", None, 0

    def _check_slots(self, net, slots, roi_layout=None, direct=None):
        """-> self.slots, self.roi_layout, self.direct (`_roi_options`), or ValueError before anything is made."""
        self.roi_layout, self.direct = _roi_options(net, type(self).__name__, roi_layout, direct)
        self.slots = [tuple(int(v) for v in s) for s in slots]
        if len(self.slots) < 1 or any(len(s) != 3 for s in self.slots):
            raise ValueError("slots: at least one (image, w, h)")
        for img, w, h in self.slots:
            if not 0 <= img < len(net.sizes):
                raise ValueError(f"slot image {img}: the net has {len(net.sizes)} images")
            if w < 1 or h < 1 or w > net.sizes[img][0] or h > net.sizes[img][1]:
                raise ValueError(f"a {w} x {h} rectangle is empty or larger than the {net.sizes[img][0]} x {net.sizes[img][1]} image")

    def _make(self, net, c):
        """The library object over the coder `c` of `net`'s latents, the window net and the tensors."""
        import torch
        L, n = _lib.lib(), len(self.slots)
        self.device = net.device
        self._cslots = (_lib.RaggedRoiSlot * n)(*[_lib.RaggedRoiSlot(*s) for s in self.slots])
        self.layout = (self._slot_type * n)()
        totals = (ctypes.c_uint64 * self._n_totals)()
        _lib.check(getattr(L, self._abi + "_layout")(c._lat_w, c._lat_h, c.lat_c, c._wss, c._img_w, c._img_h, len(c.shapes), self._cslots, n,
                                                     self.layout, totals), self._abi + "_layout")
        self.band_bytes, self.latent_bytes, self.recon_bytes, self.roi_bytes, ws_bytes = (int(v) for v in totals[:5])
        self.items = int(totals[5]) if self._n_totals == 6 else tuple(int(v) for v in totals[5:])
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(getattr(L, self._abi + "_create")(c._h, self._cslots, n, ctypes.byref(self._h)), self._abi + "_create")
        # the window net: layers 4 .. on `net`'s weights, descs and GDN objects over the sizes (16 cw_cap, 16 rh_cap); direct: with
        # the rectangles (0, 0, w, h) of the slots, moved on every decode to the origins the place kernel leaves in the object
        self.window_net = RaggedNet([(16 * int(s.cw_cap), 16 * int(s.rh_cap)) for s in self.layout], device=self.device,
                                    shared_weights=net.weights, descs=net.descs, gdn=net.gdn,
                                    **(dict(out_rects=[(0, 0, w, h) for _, w, h in self.slots], out_layout=self.roi_layout)
                                       if self.direct else {}))
        self._last = len(net.descs) - 1
        if self.window_net.nbytes(3) != self.latent_bytes or self.window_net.nbytes(self._last) != (self.roi_bytes if self.direct
                                                                                                   else self.recon_bytes):
            raise RuntimeError("the window net's tensors are not the layout's")
        if self.direct and self.window_net._offsets[self._last + 1] != [int(s.roi_offset) for s in self.layout]:
            raise RuntimeError("the window net's rectangles do not lie where the layout puts the ROI pixels")
        self._origins = ctypes.c_void_p(getattr(L, self._abi + "_origins")(self._h)) if self.direct else None
        self.window_net.workspace()
        u8 = dict(dtype=torch.uint8, device=self.device)
        self.band = torch.empty(max(self.band_bytes, 16), **u8)
        self.latent = torch.empty(self.latent_bytes, **u8)
        self.recon = None if self.direct else torch.empty(self.recon_bytes, **u8)
        self.roi = torch.empty(self.roi_bytes, **u8)
        self.ws = torch.empty(max(int(getattr(L, self._abi + "_workspace_bytes")(self._h)), ws_bytes, 256), **u8)
        self.status = torch.zeros((n, 2), dtype=torch.int32, device=self.device)
        self.flags = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.xy = torch.zeros((n, 2), dtype=torch.int32, device=self.device)      # where a host sequence of positions is copied
        self.uniform = len({(w, h) for _, w, h in self.slots}) == 1

    def _positions(self, xy, stream):
        """xy as `decode` takes it -> the device tensor the kernels read: xy itself, or the object's own after a copy on the stream."""
        import torch
        n = len(self.slots)
        if isinstance(xy, torch.Tensor) and xy.is_cuda:
            if not (xy.dtype == torch.int32 and xy.is_contiguous() and tuple(xy.shape) == (n, 2)):
                raise TypeError(f"xy as a tensor: a contiguous CUDA int32 tensor of shape ({n}, 2)")
            return xy
        host = np.asarray(xy)
        if host.shape != (n, 2) or host.dtype.kind not in "iu" or host.min() < -2 ** 31 or host.max() >= 2 ** 31:
            raise ValueError(f"xy: one int32 (x0, y0) per slot, {n}")
        with torch.cuda.stream(stream if isinstance(stream, torch.cuda.Stream) else None):
            self.xy.copy_(torch.from_numpy(host.astype(np.int32)))
        return self.xy

    def _decode(self, xy, out, stream, *coder_args):
        """The placed decode (`coder_args`: what `<_abi>_decode_async` takes between the positions and the band), the window net and
        the pixel cut -> `out` or the object's own pixels."""
        out = self.roi if out is None else out
        _check_tensor(out, (self.roi_bytes,), "out")
        L, sp, vp = _lib.lib(), _stream_ptr(stream), ctypes.c_void_p
        _lib.check(getattr(L, self._abi + "_decode_async")(
            self._h, vp(xy.data_ptr()), *coder_args, vp(self.band.data_ptr()), vp(self.latent.data_ptr()), vp(self.status.data_ptr()),
            vp(self.flags.data_ptr()), vp(self.ws.data_ptr()), self.ws.numel(), sp), self._abi + "_decode_async")
        if self.direct:
            # layer 7 stores the placed rectangles itself, at the origins the place kernel has just written on this stream
            self.window_net.run_layers(4, self._last, self.latent, out=out, stream=stream, origins=self._origins)
        else:
            self.window_net.run_layers(4, self._last, self.latent, out=self.recon, stream=stream)
            _lib.check(getattr(L, self._abi + "_cut_async")(self._h, vp(self.recon.data_ptr()), vp(out.data_ptr()), sp),
                       self._abi + "_cut_async")
        if self.uniform:
            _, w, h = self.slots[0]
            return out.view(len(self.slots), *((3, h, w) if self.roi_layout == "planar" else (h, w, 3)))
        return out

    def views(self, roi):
        """Per-slot [h][w][3] views of what `decode` returned ([3][h][w] with roi_layout="planar")."""
        flat = roi.reshape(-1)
        _check_tensor(flat, (self.roi_bytes,), "roi")
        return [flat[int(s.roi_offset):int(s.roi_offset) + h * w * 3].view(*((3, h, w) if self.roi_layout == "planar" else (h, w, 3)))
                for s, (_, w, h) in zip(self.layout, self.slots)]


class MovingRoi(_MovingRoiChain):
    """Pixel rectangles of fixed SIZE whose POSITIONS are read from device memory on every call (include/sicn_ragged_roi_move.h):
    made once for a list of slots, `decode(xy)` then costs its nine launches and nothing else — no allocation, no upload of tables,
    no host synchronisation — so a captured graph replays with new positions and a loader can draw them on the device.
    slots: (image, w, h) per slot, `image` an index into the net's batch; several slots may name one image, in any order.
    coder: the RaggedLatentCoder whose slots hold the containers (default: a new one from net.latent_coder(stream_symbols)); after
    `RaggedArchive.unpack(images=...)` into it, an archive serves any number of moves.  Same bytes as the full decode, sliced; a
    position outside [0, image - size] is clamped and bit 0 of the slot's `.flags` word says so.
    `.status`: device int32 [n_slots][2], the window decoder's verdicts per slot; `.flags`: device int32 [n_slots].
    roi_layout, direct: see `_roi_options`.  With `direct`, layer 7 of the window net stores the placed rectangles itself, at the
    origins the placement leaves on the device — eight launches, `recon` is None and no pixel cut runs."""
    _free, _abi, _slot_type, _n_totals = "sicn_ragged_roi_move_free", "sicn_ragged_roi_move", _lib.RaggedRoiMoveSlot, 6

    def __init__(self, net, slots, coder=None, stream_symbols=16384, roi_layout=None, direct=None):
        self.net = net
        self._check_slots(net, slots, roi_layout, direct)
        self.coder = c = coder if coder is not None else net.latent_coder(stream_symbols)
        lat = net.shapes(3)
        if [(h, w) for h, w, _ in lat] != c.shapes or lat[0][2] != c.lat_c or c.image_sizes != net.sizes:
            raise ValueError("the coder's latent shapes or image sizes are not the net's")
        self._make(net, c)

    def decode(self, xy, slots=None, valid=None, stream=None, out=None):
        """xy: the positions (x0, y0) per slot — a CUDA int32 tensor [n_slots][2], read when the kernels run, or a host sequence,
        which is copied into the object's own device tensor on the stream.  slots, valid: as in RaggedLatentCoder.decode.  Returns
        the ROI pixels: `out` (a flat tensor of roi_bytes; default the object's own), as [n_slots][h][w][3] where all slots have one
        size, flat otherwise (`views` gives them per slot).  Enqueue only: nine launches, nothing allocated."""
        c = self.coder
        xy = self._positions(xy, stream)
        slots = c.slot_buffer if slots is None else slots
        c._flat(slots, c.slot_bytes, "slots")
        from .codec import _valid_ptr
        return self._decode(xy, out, stream, ctypes.c_void_p(slots.data_ptr()), _valid_ptr(c.enc_status, slots is c.slot_buffer, valid))

    def place(self, xy):
        """Host arithmetic (sicn_ragged_roi_move_place): per slot the dict {x0, y0 after the clamp, c0, r0, cw, rh, x, y, flags}."""
        out = []
        for (img, w, h), (x0, y0) in zip(self.slots, xy):
            (lh, lw), (iw, ih) = self.coder.shapes[img], self.net.sizes[img]
            p = _lib.RaggedRoiPlaced()
            _lib.check(_lib.lib().sicn_ragged_roi_move_place(4, iw, ih, lw, lh, w, h, int(x0), int(y0), ctypes.byref(p)),
                       "sicn_ragged_roi_move_place")
            out.append({k: int(getattr(p, k)) for k, _ in _lib.RaggedRoiPlaced._fields_})
        return out


class RaggedNet(_lib.Handle):
    """A layer chain over images of DIFFERENT sizes, one kernel launch per layer for the whole batch (include/sicn_ragged.h); by
    default the 8-layer chain.  `sizes`: [(width, height)] per image at the chain's input.  A ragged tensor is a flat uint8 CUDA
    tensor: the images' [H][W][C] arrays back to back; `layer` -1 names the input, l the output of layer l.  Same bytes as
    `EightLayersNet(w, h).forward` of every image alone.
    `descs`: any chain the ragged kernels serve instead of the eight layers (its spatial fields are ignored; `params` or
    `shared_weights` must match it, as in `EightLayersNet(descs=...)`).  `gdn`: a list of `GDN | None`, one per layer — the
    activation in place of that layer's ReLU (sicn_ragged_net_create_gdn); one more launch per such layer, for the whole batch.
    `rgb_ends`: "packed" (default) runs a conv 3 -> N and a deconv N -> 3 of the chain on the packed-K kernels of
    include/sicn_ragged_rgb.h, "generic" on the channel-generic ones like every other layer; the bytes are the same.
    `rgb_layout`: "interleaved" (default) or "planar" (include/sicn_ragged_planar.h).  With "planar" the input is [3][h][w] per image
    if the chain begins with a conv 3 -> N, and the output is [3][h][w] if it ends with a deconv N -> 3: `shapes`, `nbytes`, `pack`
    and `views` of those boundaries follow, everything else is unchanged.  `out_sizes`: [(width, height)] of the planar output, each
    within the chain-rule size — the top-left corner of every reconstruction is stored, nothing else.  None: the images' sizes where
    the chain begins with a conv 3 -> N and every image fits its reconstruction (the eight layers: no `cropped` pass is needed),
    the chain-rule sizes otherwise.  An end of the chain that is not such a layer stays as it is: on a chain with neither, "planar"
    makes the interleaved net (`planar_in`, `planar_out` say which ends are planar).
    `out_rects`: [(x0, y0, w, h)] per image (include/sicn_ragged_rect.h), with either `rgb_layout`, exclusive with `out_sizes`: the
    last layer — a deconv N -> 3 without an activation of its own — stores that rectangle of every reconstruction and nothing else,
    [h][w][3] or [3][h][w] per image; `shapes`, `nbytes`, `views`, `pack` and `kernel_for` of the last boundary follow, and
    `run_layers(origins=)` moves the rectangles.  `out_layout`: the layout of that output where it is not `rgb_layout`'s (a window
    net writes planar rectangles while its own input end, which it never runs, stays as it is)."""
    _free = "sicn_ragged_net_free"

    def __init__(self, sizes, params=None, device=None, n_ch: int = 128, m_ch: int = 192,
                 shared_weights: Optional[Sequence[DeviceWeights]] = None, descs: Optional[Sequence[LayerDesc]] = None,
                 gdn: Optional[Sequence[Optional["GDN"]]] = None, rgb_ends: str = "packed", rgb_layout: str = "interleaved",
                 out_sizes=None, out_rects=None, out_layout: Optional[str] = None):
        import torch
        if rgb_ends not in _lib.RAGGED_RGB_ENDS:
            raise ValueError(f"rgb_ends: 'packed' or 'generic', not {rgb_ends!r}")
        if rgb_layout not in _lib.RAGGED_PIXELS:
            raise ValueError(f"rgb_layout: 'interleaved' or 'planar', not {rgb_layout!r}")
        if rgb_layout == "planar" and rgb_ends != "packed":
            raise ValueError("rgb_layout='planar' needs rgb_ends='packed': the generic family has no planar form")
        self.rgb_ends, self.rgb_layout = rgb_ends, rgb_layout
        L = _lib.lib()
        self.sizes = [(int(w), int(h)) for w, h in sizes]
        n_img = len(self.sizes)
        w0, h0 = self.sizes[0] if self.sizes else (1, 1)
        # the library ignores the descriptors' spatial fields
        self.descs: List[LayerDesc] = list(descs) if descs is not None else eight_layer_descs(max(w0, 1), max(h0, 1), n_ch, m_ch)
        self.device = torch.device(device if device is not None else "cuda")
        if shared_weights is not None:
            self.weights = list(shared_weights)
        else:
            params = params if params is not None else load_param_weights()
            with torch.cuda.device(self.device):
                self.weights = [DeviceWeights(d, w, b) for d, (w, b) in zip(self.descs, params)]
        n = len(self.descs)
        planar = rgb_layout == "planar" and n > 0
        self.planar_in = planar and not self.descs[0].transposed and self.descs[0].IFM_CH == 3
        self.planar_out = planar and bool(self.descs[-1].transposed) and self.descs[-1].OFM_CH == 3
        if out_sizes is not None and not self.planar_out:
            raise ValueError("out_sizes: only a planar output (rgb_layout='planar', a chain that ends with deconv N -> 3) has sizes of its own")
        if out_sizes is None and out_rects is None and self.planar_out and self.planar_in:
            chain = self.sizes
            for d in self.descs:
                chain = [(2 * w, 2 * h) if d.transposed else (-(-w // 2), -(-h // 2)) for w, h in chain]
            if all(w <= cw and h <= ch for (w, h), (cw, ch) in zip(self.sizes, chain)):
                out_sizes = self.sizes
        if out_rects is not None:
            if out_sizes is not None:
                raise ValueError("out_rects and out_sizes exclude each other: a rectangle has its own size")
            if rgb_ends != "packed":
                raise ValueError("out_rects needs rgb_ends='packed': the generic family has no rectangle form")
            if out_layout is not None and out_layout not in _lib.RAGGED_PIXELS:
                raise ValueError(f"out_layout: 'interleaved' or 'planar', not {out_layout!r}")
            if not (n > 0 and self.descs[-1].transposed and self.descs[-1].OFM_CH == 3):
                raise ValueError("out_rects: the chain must end with a deconv N -> 3")
            if gdn is not None and len(gdn) == n and gdn[-1] is not None:
                raise ValueError("out_rects: the last layer must not carry a GDN / IGDN")
            self.out_rects = [tuple(int(v) for v in r) for r in out_rects]
            if len(self.out_rects) != len(self.sizes) or any(len(r) != 4 for r in self.out_rects):
                raise ValueError(f"out_rects: one (x0, y0, w, h) per image, {len(self.sizes)}")
            if out_layout is not None:
                self.planar_out = out_layout == "planar"
        else:
            if out_layout is not None:
                raise ValueError("out_layout: only with out_rects")
            self.out_rects = None
        self.out_sizes = None if out_sizes is None else [(int(w), int(h)) for w, h in out_sizes]
        if self.out_sizes is not None and len(self.out_sizes) != len(self.sizes):
            raise ValueError(f"out_sizes: one (width, height) per image, {len(self.sizes)}")
        self._cdescs = (CLayerDesc * n)(*[d.to_c() for d in self.descs])
        self._widths = (ctypes.c_int32 * max(n_img, 1))(*[w for w, _ in self.sizes])
        self._heights = (ctypes.c_int32 * max(n_img, 1))(*[h for _, h in self.sizes])
        handles = (ctypes.c_void_p * n)(*[w.handle for w in self.weights])
        self._h = ctypes.c_void_p()
        self.gdn = list(gdn) if gdn is not None else None      # keeps the activations alive
        if self.gdn is not None and len(self.gdn) != n:
            raise ValueError("gdn must have one entry (or None) per layer")
        ghandles = None
        if self.gdn is not None:
            ghandles = (ctypes.c_void_p * n)(*[(g.handle if g is not None else None) for g in self.gdn])
        self._out_widths = self._out_heights = None
        if self.out_sizes is not None:
            self._out_widths = (ctypes.c_int32 * max(n_img, 1))(*[w for w, _ in self.out_sizes])
            self._out_heights = (ctypes.c_int32 * max(n_img, 1))(*[h for _, h in self.out_sizes])
        self._crects = None
        if self.out_rects is not None:
            self._crects = (_lib.RaggedRect * max(n_img, 1))(*[_lib.RaggedRect(*r) for r in self.out_rects])
            rc = L.sicn_ragged_rect_layout(self._cdescs, n, self._widths, self._heights, n_img, self._crects, 0, (ctypes.c_int64 * 5)())
            if rc == -22:
                raise ValueError(f"out_rects {self.out_rects}: a rectangle is empty, has a negative corner or reaches beyond its reconstruction")
        with torch.cuda.device(self.device):
            if self.out_rects is not None:
                _lib.check(L.sicn_ragged_net_create_rect(self._cdescs, handles, ghandles, n, self._widths, self._heights, n_img,
                                                         _lib.RAGGED_RGB_ENDS[rgb_ends], int(self.planar_in), int(self.planar_out),
                                                         self._crects, ctypes.byref(self._h)), "sicn_ragged_net_create_rect")
            else:
                _lib.check(L.sicn_ragged_net_create_planar(self._cdescs, handles, ghandles, n, self._widths, self._heights, n_img,
                                                           _lib.RAGGED_RGB_ENDS[rgb_ends], int(self.planar_in), int(self.planar_out),
                                                           self._out_widths, self._out_heights, ctypes.byref(self._h)),
                           "sicn_ragged_net_create_planar")
        # per boundary (-1 .. n - 1, index layer + 1): the images' shapes and byte offsets, as the library lays them out
        self._shapes, self._offsets, self._nbytes = [], [], []
        q = (ctypes.c_int64 * 8)()
        for layer in range(-1, n):
            shapes, offs = [], []
            for i in range(n_img):
                _lib.check(L.sicn_ragged_layout(self._cdescs, n, self._widths, self._heights, n_img, layer, i, q), "sicn_ragged_layout")
                shapes.append((int(q[1]), int(q[0]), int(q[2])))
                offs.append(int(q[3]))
            self._shapes.append(shapes)
            self._offsets.append(offs)
            self._nbytes.append(int(q[4]))
        # a planar boundary: (3, h, w) per image; the output at its own sizes and offsets (sicn_ragged_planar_layout)
        if self.planar_in:
            self._shapes[0] = [(c, h, w) for h, w, c in self._shapes[0]]
        if self.out_rects is not None:
            shapes, offs, q5 = [], [], (ctypes.c_int64 * 5)()
            self.live_tiles = []        # per image: the tiles of the last layer that meet the rectangle at the creation's origin
            for i in range(n_img):
                _lib.check(L.sicn_ragged_rect_layout(self._cdescs, n, self._widths, self._heights, n_img, self._crects, i, q5),
                           "sicn_ragged_rect_layout")
                shapes.append((3, int(q5[1]), int(q5[0])) if self.planar_out else (int(q5[1]), int(q5[0]), 3))
                offs.append(int(q5[2]))
                self.live_tiles.append(int(q5[4]))
            self._shapes[n], self._offsets[n], self._nbytes[n] = shapes, offs, int(q5[3])
        elif self.planar_out:
            shapes, offs = [], []
            for i in range(n_img):
                _lib.check(L.sicn_ragged_planar_layout(self._cdescs, n, self._widths, self._heights, n_img, 1, self._out_widths,
                                                       self._out_heights, i, q), "sicn_ragged_planar_layout")
                shapes.append((3, int(q[1]), int(q[0])))
                offs.append(int(q[2]))
            self._shapes[n], self._offsets[n], self._nbytes[n] = shapes, offs, int(q[3])
        self._ws = None
        self._coders = {}           # compress()'s RaggedLatentCoders by stream length, made on first use
        self._archives = {}         # compress_archive()'s RaggedArchives, one per coder
        self._crop = None           # cropped()'s RaggedCrop, made on first use
        self._rois = {}             # decompress_archive(rois=)'s RaggedRoi objects by coder and rectangles
        self._last_roi = None

    def shapes(self, layer: int):
        """[(H, W, C)] of every image at boundary `layer`; [(3, H, W)] at a planar one."""
        return list(self._shapes[layer + 1])

    def nbytes(self, layer: int) -> int:
        return self._nbytes[layer + 1]

    def kernel_for(self, layer: int) -> str:
        """The kernel `layer` runs on (sicn_ragged_net_kernel_for): "mfma_conv_any", "mfma_deconv_any", "mfma_conv_rgb_packed" or
        "mfma_deconv_rgb_packed"; "mfma_conv_rgb_planar" and "mfma_deconv_rgb_planar" at a planar boundary;
        "mfma_deconv_rgb_rect" and "mfma_deconv_rgb_planar_rect" for the last layer of a net with `out_rects`."""
        name = _lib.lib().sicn_ragged_net_kernel_for(self._h, int(layer))
        if name is None:
            raise ValueError("layer out of range")
        return name.decode()

    def pack(self, images, layer: int = -1):
        """[H][W][C] uint8 tensors (any device; [3][H][W] at a planar boundary), one per image -> the ragged tensor of boundary
        `layer` on the net's device."""
        import torch
        shapes = self._shapes[layer + 1]
        if len(images) != len(shapes):
            raise ValueError(f"need {len(shapes)} images")
        packed = torch.empty(self.nbytes(layer), dtype=torch.uint8, device=self.device)
        for t, v, shp in zip(images, self.views(layer, packed), shapes):
            if tuple(t.shape) != shp or t.dtype != torch.uint8:
                raise ValueError(f"image shape {tuple(t.shape)} / dtype {t.dtype}: need uint8 {shp}")
            v.copy_(t)
        return packed

    def views(self, layer: int, packed):
        """Per-image [H][W][C] views of a ragged tensor of boundary `layer` ([3][H][W] at a planar one; no copy; each one is
        contiguous)."""
        _check_tensor(packed, (self.nbytes(layer),), "packed")
        return [packed[o:o + a * b * c].view(a, b, c) for o, (a, b, c) in zip(self._offsets[layer + 1], self._shapes[layer + 1])]

    def workspace(self):
        import torch
        if self._ws is None:
            nbytes = max(int(_lib.lib().sicn_ragged_net_workspace_bytes(self._h)), 256)
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def run_layers(self, first: int, last: int, packed_in, tap_layer: int = -1, out=None, tap=None, stream=None, origins=None):
        """Layers [first, last] over the whole batch (sicn_ragged_net_forward_at); returns (out, tap or None), ragged tensors.
        origins: on a net with `out_rects` and with `last` the last layer, a contiguous CUDA int32 tensor [n_images][2] of (x0, y0)
        per image, read when the last layer runs, in place of the creation's origins.  Every value is admissible: the part of a
        rectangle that lies outside its reconstruction is not written."""
        import torch
        if not 0 <= first <= last < len(self.descs):
            raise ValueError("layer range")
        origins_ptr = ctypes.c_void_p(0)
        if origins is not None:
            if self.out_rects is None or last != len(self.descs) - 1:
                raise ValueError("origins: only on a net made with out_rects, and only when the last layer runs")
            if isinstance(origins, ctypes.c_void_p):        # the table a moving ROI object owns (sicn_ragged_roi_move_origins)
                origins_ptr = origins
            elif not (isinstance(origins, torch.Tensor) and origins.is_cuda and origins.dtype == torch.int32 and origins.is_contiguous()
                      and tuple(origins.shape) == (len(self.sizes), 2)):
                raise TypeError(f"origins: a contiguous CUDA int32 tensor of shape ({len(self.sizes)}, 2)")
            else:
                origins_ptr = ctypes.c_void_p(origins.data_ptr())
        _check_tensor(packed_in, (self.nbytes(first - 1),), "in")
        if out is None:
            out = torch.empty(self.nbytes(last), dtype=torch.uint8, device=packed_in.device)
        _check_tensor(out, (self.nbytes(last),), "out")
        tap_ptr = ctypes.c_void_p(0)
        if tap_layer >= 0:
            if tap is None:
                tap = torch.empty(self.nbytes(tap_layer), dtype=torch.uint8, device=packed_in.device)
            _check_tensor(tap, (self.nbytes(tap_layer),), "tap")
            tap_ptr = ctypes.c_void_p(tap.data_ptr())
        else:
            tap = None
        ws = self.workspace()
        _lib.check(_lib.lib().sicn_ragged_net_forward_at(self._h, first, last, ctypes.c_void_p(packed_in.data_ptr()),
                                                         ctypes.c_void_p(out.data_ptr()), tap_layer, tap_ptr,
                                                         ctypes.c_void_p(ws.data_ptr()), ws.numel(), origins_ptr, _stream_ptr(stream)),
                   "sicn_ragged_net_forward_at")
        return out, tap

    def forward(self, packed_in, out=None, latent=None, stream=None):
        """All layers; returns (reconstructions, latents) as ragged tensors (the latent is layer 3's output)."""
        n = len(self.descs)
        return self.run_layers(0, n - 1, packed_in, tap_layer=3 if n > 3 else -1, out=out, tap=latent, stream=stream)

    def cropped(self, out, dst=None, stream=None):
        """The chain's last output (boundary n - 1, every size rounded up by the chain rule: 112 x 48 for a 100 x 36 image) cut to the
        images' own sizes: a ragged tensor laid out as boundary -1 with the output's channels.  One launch.  Needs a chain that
        ends no smaller than it began (the eight layers do).  A planar output that already has the images' sizes is returned as it
        is; one of other sizes is a ValueError (make the net with out_sizes=None)."""
        last = len(self.descs) - 1
        if self.planar_out:
            if [(w, h) for _, h, w in self.shapes(last)] != self.sizes:
                raise ValueError("the planar output has sizes of its own (out_sizes), not the images': there is no planar crop")
            if dst is not None:
                raise ValueError("dst: the planar output already has the images' sizes and is returned as it is; nothing is copied")
            _check_tensor(out, (self.nbytes(last),), "out")
            return out
        if self._crop is None:
            self._crop = RaggedCrop([(h, w) for h, w, _ in self.shapes(last)], [(h, w) for w, h in self.sizes],
                                    self.shapes(last)[0][2], device=self.device)
        return self._crop.run(out, dst, stream=stream)

    def crop_views(self, cropped):
        """Per-image [height][width][C] views of what `cropped` returned ([3][height][width] of a planar output)."""
        if self.planar_out:
            return self.views(len(self.descs) - 1, cropped)
        if self._crop is None:
            raise ValueError("cropped() has not run")
        return self._crop.views(cropped)

    def roi_views(self, roi_pixels):
        """Per-image [h][w][3] views of what the last `decompress_archive(rois=...)` returned."""
        if self._last_roi is None:
            raise ValueError("decompress_archive(rois=...) has not run")
        return self._last_roi.views(roi_pixels)

    def moving_roi(self, slots, coder=None, stream_symbols=16384, roi_layout=None, direct=None):
        """A MovingRoi over this net: `slots` = (image, w, h) per slot, positions given per `decode` call, from device memory.
        ValueError for a net with planar pixels unless `roi_layout` names the layout of the ROI pixels."""
        return MovingRoi(self, slots, coder=coder, stream_symbols=stream_symbols, roi_layout=roi_layout, direct=direct)

    def latent_coder(self, stream_symbols=None):
        """A codec.RaggedLatentCoder for this net's latents (boundary 3) and image sizes: the whole batch in 3 + 2 launches.
        ValueError where boundary 3 is a planar pixel boundary and no latent."""
        if self.planar_out and len(self.descs) == 4:
            raise ValueError("boundary 3 of this chain is its planar RGB output, not a latent")
        from . import codec
        return codec.RaggedLatentCoder([(h, w) for h, w, _ in self.shapes(3)], self.shapes(3)[0][2], self.sizes,
                                       stream_symbols=stream_symbols, device=self.device)

    def _coder_for(self, stream_symbols):
        """(key, coder): the latent coder for these stream lengths — one number, "auto", or one length per image — made on first
        use and shared by compress, compress_archive and decompress_archive: creating one costs device allocations, table uploads
        and a synchronisation.  Lengths per image are served by a coder that already has them, whatever it was asked for."""
        if isinstance(stream_symbols, (int, str)):
            key = stream_symbols
        else:
            stream_symbols = [int(v) for v in stream_symbols]
            key = next((k for k, c in self._coders.items() if c.stream_symbols == stream_symbols), None)
            if key is None:
                key = stream_symbols[0] if len(set(stream_symbols)) == 1 else tuple(stream_symbols)
        if key not in self._coders:
            self._coders[key] = self.latent_coder(stream_symbols)
        return key, self._coders[key]

    def _archive_for(self, key):
        """The one-section archive object over the coder of `key` (`_coder_for`), made on first use."""
        from . import codec
        if key not in self._archives:
            self._archives[key] = codec.RaggedArchive([self._coders[key]], tag=0, device=self.device)
        return self._archives[key]

    def compress(self, packed_in, stream_symbols=16384, stream=None):
        """Ragged input -> one rANS-W container (`bytes`) per image: layers 0-3, then the ragged encoder, enqueued back to back;
        the only host synchronisation is the read-back of the containers at the end.  stream_symbols: 16384, the format's default,
        gives the bytes of `EightLayersNet(w, h)` + `codec.encode_latent` on every image alone; "auto" or a shorter power of two
        (codec.RaggedLatentCoder) shortens the serial chain of small latents at 260 bytes per extra stream."""
        _, coder = self._coder_for(stream_symbols)
        latent, _ = self.run_layers(0, 3, packed_in, stream=stream)
        coder.encode(latent, stream=stream)
        return coder.containers()

    def decompress(self, containers, out=None, stream=None):
        """Containers of this net's images (e.g. from `compress`) -> the reconstructions as a ragged tensor of boundary 7: the ragged
        decoder, then layers 4-7, enqueued back to back.  A container that fails to decode raises when the work has finished."""
        import torch
        from . import codec
        coder = codec.RaggedLatentCoder.for_containers(containers, device=self.device)
        if [(h, w, coder.lat_c) for h, w in coder.shapes] != self.shapes(3):
            raise ValueError("the containers' latent shapes are not this net's")
        latent = torch.empty(self.nbytes(3), dtype=torch.uint8, device=self.device)
        coder.decode(latent, stream=stream)
        out, _ = self.run_layers(4, len(self.descs) - 1, latent, out=out, stream=stream)
        coder.check()
        return out

    def compress_archive(self, packed_in, stream_symbols=16384, stream=None):
        """`compress` with the batch's containers as ONE byte string (codec.RaggedArchive, tag 0): layers 0-3, the ragged encoder and
        the two launches that pack the archive on the device, enqueued back to back; exactly the archive's bytes travel to the host.
        `codec.split_archive` of the result gives `compress`'s containers."""
        key, coder = self._coder_for(stream_symbols)
        archive = self._archive_for(key)
        latent, _ = self.run_layers(0, 3, packed_in, stream=stream)
        coder.encode(latent, stream=stream)
        archive.pack(stream=stream)
        b = archive.bytes()
        archive.check()             # an image the encoder refused (bit 0) raises, as compress does
        return b

    @classmethod
    def from_archive(cls, b, images=None, **net_kwargs):
        """The net for the images an archive names — all of them, or the selection `images` (strictly ascending indices into the
        archive): the sizes are READ from the containers' headers.  `decompress_archive(b, images=images)` then reads it."""
        from . import codec
        info = codec.archive_info(b)
        sel = range(info["n_images"]) if images is None else codec._selection(images, n_archive=info["n_images"])
        sizes = [info["image_sizes"][i] for i in sel]
        if any(s is None for s in sizes):
            raise ValueError("an image of the selection has no container to read its size from")
        return cls(sizes, **net_kwargs)

    def decompress_archive(self, b, out=None, stream=None, images=None, rois=None, roi_layout=None, direct=None):
        """An archive of this net's images (e.g. from `compress_archive`) -> the reconstructions as a ragged tensor of boundary 7:
        upload, the two launches that unpack it, the ragged decoder, layers 4-7.  Raises when the work has finished if the archive
        was refused or a container fails to decode.
        `images`: the archive may hold more images than this net; a strictly ascending sequence of len(self.sizes) indices into it
        names the ones to decode (ValueError otherwise, before any launch), and the sizes and latent shapes of THOSE containers must
        be this net's.  The whole archive is uploaded, two launches copy the selected containers alone, whatever it holds.
        `rois`: one (x0, y0, w, h) per decoded image, or None for that image whole — only the streams, latent columns and pixels the
        rectangles need are decoded (RaggedRoi: eight launches behind the unpack), and the result is the ROI pixels as a ragged
        [h][w][3] tensor (`roi_views` gives them per image), the bytes of the full decode sliced.  A wrong length or a rectangle
        outside its image is a ValueError before any launch.  One rectangle per image per call: two details of one photograph are
        two calls.  The window cannot check the checksum of the whole latent; every other verdict raises as without `rois`.
        `roi_layout`, `direct` (with `rois`): as in RaggedRoi — "planar" gives [3][h][w] per image, `direct` lets layer 7 store the
        rectangles itself."""
        import torch
        from . import codec
        info = codec.archive_info(b)
        if rois is not None:
            roi_layout, direct = _roi_options(self, "decompress_archive(rois=)", roi_layout, direct)
            if len(rois) != len(self.sizes):
                raise ValueError(f"rois: one rectangle (or None) per decoded image, {len(self.sizes)}")
            rois = tuple(None if r is None else tuple(int(v) for v in r) for r in rois)
            for size, r in zip(self.sizes, rois):
                roi_plan(size, (0, 0) + size if r is None else r)
        sel = None if images is None else codec._selection(images, n_archive=info["n_images"], n_expected=len(self.sizes))
        chosen = range(info["n_images"]) if sel is None else sel
        heads = [info["headers"][i][0] for i in chosen]
        if info["n_sections"] != 1 or any(h is None or int(h.mode) != codec.RANSW for h in heads):
            raise ValueError("not an archive of one rANS-W section")
        if [info["latent_shapes"][i][0] for i in chosen] != self.shapes(3) or [info["image_sizes"][i] for i in chosen] != self.sizes:
            raise ValueError("the archive's image sizes or latent shapes are not this net's")
        key, coder = self._coder_for([int(h.stream_symbols) for h in heads])
        archive = self._archive_for(key)
        if rois is not None:
            if (key, rois, roi_layout, direct) not in self._rois:
                self._rois[(key, rois, roi_layout, direct)] = RaggedRoi(self, rois, coder=coder, roi_layout=roi_layout, direct=direct)
            roi = self._last_roi = self._rois[(key, rois, roi_layout, direct)]
            valid, = archive.unpack(b, stream=stream, images=sel)
            out = roi.decode(valid=valid, stream=stream, out=out)
            archive.check()
            _raise_on_status(roi.status[:, 0].cpu().tolist(), "rANS-W window decode")
            return out
        valid, = archive.unpack(b, stream=stream, images=sel)
        latent = torch.empty(self.nbytes(3), dtype=torch.uint8, device=self.device)
        coder.decode(latent, valid=valid, stream=stream)
        out, _ = self.run_layers(4, len(self.descs) - 1, latent, out=out, stream=stream)
        archive.check()
        # the decoder's verdicts alone: the shared coder's encoder status is another call's
        _raise_on_status(coder.dec_status[:, 0].cpu().tolist(), "rANS-W decode")
        return out


_DEFAULT_NETS = {}


def _default_net(width, height, device) -> EightLayersNet:
    key = (width, height, str(device))
    if key not in _DEFAULT_NETS:
        _DEFAULT_NETS[key] = EightLayersNet(width, height, device=device)
    return _DEFAULT_NETS[key]


def conv2d_layer0(in_, out=None, numReps: int = 1, stream=None):
    """`conv2d_layer0(in, out, numReps)` — conv_nonsquare_top.cpp:282-286: layer 0 with
    PARAM::weights_layer0 / bias_layer0; image size taken from `in_` ([numReps][H][W][3])."""
    h, w = int(in_.shape[1]), int(in_.shape[2])
    net = _default_net(w, h, in_.device)
    return conv2d(net.descs[0], net.weights[0], None, in_, out, numReps, stream)


def deconv2d_layer4(in_, out=None, numReps: int = 1, stream=None):
    """`deconv2d_layer4(in, out, numReps)` — conv_nonsquare_top.cpp:288-291 (PARAM layer 4)."""
    h, w = int(in_.shape[1]), int(in_.shape[2])
    d = replace(REFERENCE_DESCS[4], IFM_ROW=w, IFM_COL=h, OFM_ROW=2 * w, OFM_COL=2 * h)
    net = _default_net(16 * w, 16 * h, in_.device)
    return deconv522(d, net.weights[4], None, in_, out, numReps, stream)


def eight_layers_net(in_, out=None, numReps: int = 1, stream=None):
    """`eight_layers_net(in, out, numReps)` — conv_nonsquare_top.cpp:295-357 with the PARAM tables."""
    h, w = int(in_.shape[1]), int(in_.shape[2])
    net = _default_net(w, h, in_.device)
    return net.forward(in_, out, numReps=numReps, want_latent=False, stream=stream)[0]
