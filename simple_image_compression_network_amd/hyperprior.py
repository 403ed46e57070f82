"""The hyperprior configuration (BASELINE.json configs[4]) assembled from this package's pieces.

EXTENSION BEYOND THE REFERENCE, parity UNPINNED: the reference has no GDN, no hyperprior, no context model and no coder
(SURVEY.md §0).  Everything here is built from operators that DO mirror the reference — `conv2d<>` / `deconv522<>` layers
chained by `sicn_net` — plus this project's own fixed-point GDN (include/sicn_gdn.h) and coders (include/sicn_codec.h):

    main analysis   g_a : x  -> y    L0..L3 of eight_layers_net, GDN in place of the ReLU after L0, L1, L2
    hyper analysis  h_a : y  -> z    conv2d 192->128, conv2d 128->128          (5x5, stride 2, the reference layer template)
    z bitstream               : container mode 3 (rANS-W, one static table measured on z)
    hyper synthesis h_s : z  -> s    deconv522 128->128, deconv522 128->192, cropped to y's shape: the SCALE MAP
    y bitstream               : container mode 4 (rANS-WC: 16 class tables, class from s and — for the non-anchor half of a
                                checkerboard — from the already decoded anchor neighbours)
    main synthesis  g_s : y  -> x^   L4..L7, IGDN after L4, L5, L6

The decoder derives s from the decoded z, the encoder from z itself: the z coder is lossless over bytes, so the two are the same tensor
whenever the container fits its slot (and when it does not, the encoder's status says so and nothing downstream is valid anyway).
`HyperpriorCodec(verify_z=True)` makes the encoder decode its own z container first and use THAT (rounds 2 - 4 always did; it is a
self-check of the coder inside every encode, 0.05 ms of an 8 x 4K step, not something the format needs).
All of it is kernel launches on one stream: no host synchronisation between the stages (verdicts stay on the device until
`check()`), so a whole encode + decode can be enqueued back to back or captured in a hipGraph.

Weights: the main transform uses the PARAM tables (memdata_nonsquare.h); the hyper stacks and the GDN parameters have no
reference values and are seeded random (the reference's own weights are placeholders too)."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import api, codec
from .config import LayerDesc

__all__ = ["HyperpriorCodec", "RaggedHyperpriorCodec", "RaggedHyperpriorRoi", "MovingHyperpriorRoi", "random_gdn_params", "random_layer_params", "hyper_descs", "hyper_parameters"]


def random_gdn_params(rng, channels: int):
    """beta ~ 1.0 in Q8, sparse small gamma: keeps GDN outputs spread over the int8 range."""
    beta = rng.integers(128, 1024, channels).astype(np.uint32)
    gamma = rng.integers(0, 8, (channels, channels)).astype(np.uint8)
    gamma[rng.random((channels, channels)) < 0.7] = 0
    return beta, gamma


def _pack(w_okkc: np.ndarray, simd: int, pe: int) -> np.ndarray:
    """W[o][ky][kx][c] nibbles -> FixedPointWeights words [PE][TILES] (weights.hpp:110-150; o = nf*PE + pe, k = sf*SIMD + s)."""
    cout, _, _, cin = w_okkc.shape
    kk = 25 * cin
    sf_n, nf_n = kk // simd, cout // pe
    nib = (w_okkc.reshape(nf_n, pe, sf_n, simd).astype(np.int16) & 15).astype(np.uint64)
    shifts = np.arange(simd, dtype=np.uint64) * np.uint64(4)
    words = (nib << shifts[None, None, None, :]).sum(axis=3, dtype=np.uint64)
    return np.ascontiguousarray(words.transpose(1, 0, 2).reshape(pe, nf_n * sf_n))


def random_layer_params(rng, d: LayerDesc):
    """(weights, bias) as api.FixedPointWeights, seeded random nibbles / bytes; also returns the numpy (W, b) for checkers."""
    w = rng.integers(-8, 8, (d.OFM_CH, 5, 5, d.IFM_CH)).astype(np.int8)
    b = rng.integers(-128, 128, d.OFM_CH).astype(np.int8)
    fw = api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, _pack(w, d.SIMD, d.PE))
    fb = api.FixedPointWeights(1, 8, 1, d.OFM_CH, b.view(np.uint8).astype(np.uint64))
    return (fw, fb), (w, b)


def hyper_descs(lat_w: int, lat_h: int):
    """([h_a descs], [h_s descs]) for a latent of lat_h x lat_w x 192."""
    mk = LayerDesc.make
    a0 = mk(192, 128, 12, 16, lat_w, lat_h, 0)
    a1 = mk(128, 128, 8, 16, a0.OFM_ROW, a0.OFM_COL, 0)
    s0 = mk(128, 128, 8, 16, a1.OFM_ROW, a1.OFM_COL, 1)
    s1 = mk(128, 192, 8, 24, s0.OFM_ROW, s0.OFM_COL, 1)
    return [a0, a1], [s0, s1]


def hyper_parameters(width: int, height: int, seed: int = 0, use_gdn: bool = True):
    """Every seeded parameter of the configuration, host side only (numpy; no GPU): what HyperpriorCodec uploads and what a checker
    needs to restate the pipeline (tests/golden/make_hyper_hashes.py, tests/test_hyperprior.py).  Returns a dict:
    gdn_np [8] of None | (beta, gamma, inverse, shift); da, ds: the hyper stacks' descs; pa, ps: their (weights, bias) tables;
    ha_np, hs_np: the same as (W[o][ky][kx][c], b).  ONE generator, drawn in this order — the order is part of the seed's meaning."""
    rng = np.random.default_rng(seed)
    descs = api.eight_layer_descs(width, height)
    gdn_np = [None] * 8
    if use_gdn:
        for l in (0, 1, 2, 4, 5, 6):
            beta, gamma = random_gdn_params(rng, descs[l].OFM_CH)
            gdn_np[l] = (beta, gamma, l >= 4, 12)
    lat_h, lat_w, _ = descs[3].out_shape
    da, ds = hyper_descs(lat_w, lat_h)
    pa, ha_np = zip(*[random_layer_params(rng, d) for d in da])
    ps, hs_np = zip(*[random_layer_params(rng, d) for d in ds])
    return {"gdn_np": gdn_np, "da": da, "ds": ds, "pa": list(pa), "ps": list(ps), "ha_np": list(ha_np), "hs_np": list(hs_np)}


class HyperpriorCodec:
    def __init__(self, width: int, height: int, n_images: int, seed: int = 0, device="cuda", use_gdn: bool = True,
                 main_params=None, options=None, z_stream_symbols=None, verify_z: bool = False, y_stream_symbols=None):
        import torch
        self.n, self.width, self.height = int(n_images), int(width), int(height)
        self.verify_z = bool(verify_z)
        self.device = torch.device(device)
        hp = hyper_parameters(width, height, seed, use_gdn)
        self.gdn_np = hp["gdn_np"]
        gdn = [None if g is None else api.GDN(g[0], g[1], inverse=g[2], shift=g[3]) for g in self.gdn_np]
        self.main = api.EightLayersNet(width, height, params=main_params, device=self.device, gdn=gdn if use_gdn else None,
                                       options=options)
        lat_h, lat_w, lat_c = self.main.descs[3].out_shape
        da, ds, pa, ps = hp["da"], hp["ds"], hp["pa"], hp["ps"]
        self.ha_np, self.hs_np = hp["ha_np"], hp["hs_np"]
        self.h_a = api.EightLayersNet(descs=da, params=list(pa), device=self.device, options=options)
        self.h_s = api.EightLayersNet(descs=ds, params=list(ps), device=self.device, options=options)
        zh, zw, zc = da[-1].out_shape
        n = self.n
        u8 = dict(dtype=torch.uint8, device=self.device)
        self.y = torch.empty((n, lat_h, lat_w, lat_c), **u8)
        self.z = torch.empty((n, zh, zw, zc), **u8)
        self.z_hat = torch.empty_like(self.z)
        self.s_full = torch.empty((n,) + ds[-1].out_shape, **u8)     # 2 * ceil(./2) >= the latent's size: cropped below
        self.s = torch.empty_like(self.y)
        self.y_hat = torch.empty_like(self.y)
        # the hyper-latent is small (4K: 261 k symbols): codec.auto_stream_symbols picks its stream length from ONE image's latent,
        # so a container set written by a batch of 8 decodes in a batch of 1; `z_stream_symbols` overrides it and is
        # then part of the format the decoder must be built with
        self.z_coder = codec.LatentCoder(n, zh, zw, zc, width, height, device=self.device, stream_symbols=z_stream_symbols or "auto")
        # the stream length of y (rANS-WC): None = 16384; like z's it is part of the format the decoder must be built with
        self.y_coder = codec.ContextCoder(n, lat_h, lat_w, lat_c, width, height, device=self.device, stream_symbols=y_stream_symbols)
        for net in (self.main, self.h_a, self.h_s):
            net.workspace(n)

    def _scale_map(self, z):
        """h_s(z) cropped to the latent's shape (deconv doubles a size that conv rounded up)."""
        self.h_s.run_layers(0, 1, z, out=self.s_full)
        n, h, w, c = self.y.shape
        _, hs, ws, _ = self.s_full.shape
        # one launch for the batch (torch's strided copy_ was one D2D memcpy per image: ~0.8 ms of an 8 x 4K encode + decode step)
        api._lib.check(api._lib.lib().sicn_crop_nhwc(ctypes.c_void_p(self.s_full.data_ptr()), ctypes.c_void_p(self.s.data_ptr()), n, hs,
                                                     ws, h, w, c, api._stream_ptr(None)), "sicn_crop_nhwc")
        return self.s

    def encode(self, x):
        """x: CUDA uint8 [n][H][W][3] -> two sets of containers (self.z_coder.slots, self.y_coder.slots). Enqueue only."""
        self.main.analysis(x, self.y)
        self.h_a.run_layers(0, 1, self.y, out=self.z)
        self.z_coder.encode(self.z)
        # the model must be the one the decoder can rebuild: h_s of the hyper-latent the container holds — which IS z (lossless coder);
        # verify_z decodes the container to prove it on every call
        if self.verify_z:
            self.z_coder.decode(self.z_hat)
        self.y_coder.encode(self.y, self._scale_map(self.z_hat if self.verify_z else self.z))
        return self.z_coder.slots, self.y_coder.slots

    def decode(self, out, z_slots=None, y_slots=None, z_valid=None, y_valid=None):
        """containers -> reconstruction `out` [n][H'][W'][3]. Enqueue only.  z_valid / y_valid: the encoder's status arrays
        (device int32 [n][2], `.bytes` bounds each container) when they travelled with external slots; without them an
        external slot is trusted as a whole (the container header is validated either way)."""
        self.z_coder.decode(self.z_hat, slots=z_slots, valid=z_valid)
        self.y_coder.decode(self.y_hat, self._scale_map(self.z_hat), slots=y_slots, valid=y_valid)
        self.main.synthesis(self.y_hat, out)
        return out

    def check(self):
        self.z_coder.check()
        self.y_coder.check()

    def bytes_per_image(self):
        return [a + b for a, b in zip(self.z_coder.sizes(), self.y_coder.sizes())]


class RaggedHyperpriorCodec:
    """The same configuration over n images of n DIFFERENT sizes (`sizes`: [(width, height)]), every stage one set of launches for the
    whole batch (include/sicn_ragged.h, sicn_ragged_codec.h, sicn_ragged_ctx.h):

        main, h_a, h_s : api.RaggedNet (GDN / IGDN layers: the layer kernel, then the activation over the whole boundary tensor)
        z bitstream     : codec.RaggedLatentCoder, 3 launches to encode and 2 to decode
        scale map       : api.RaggedCrop cuts h_s(z), 4 * ceil(./4) per image, to every latent's own shape in one launch
        y bitstream     : codec.RaggedContextCoder, 6 launches to encode and 8 to decode, fed the ragged y, s and y_hat as they lie

    Image i's containers are `HyperpriorCodec(w_i, h_i, 1, seed)`'s, byte for byte: hyper_parameters draws depend on channel counts
    only, so every image gets that codec's parameters.  Stage tensors (y, z, z_hat, s, y_hat) are ragged tensors; `main.views(3, y)`,
    `h_a.views(1, z)` give the per-image arrays.  Parity UNPINNED, as everything in this module.
    `rgb_layout`: handed to `main` (api.RaggedNet): with "planar", `encode` takes the planar ragged input and `decode` returns the
    planar reconstructions at the images' sizes; containers and archives are the interleaved codec's bytes; `roi` and `moving_roi`
    raise ValueError."""

    def __init__(self, sizes, seed: int = 0, device="cuda", use_gdn: bool = True, main_params=None, z_stream_symbols=None,
                 y_stream_symbols=None, rgb_layout: str = "interleaved"):
        import torch
        self.sizes = [(int(w), int(h)) for w, h in sizes]
        if not self.sizes:
            raise ValueError("no images")
        self.device = torch.device(device)
        hp = hyper_parameters(*self.sizes[0], seed, use_gdn)
        self.gdn_np = hp["gdn_np"]
        with torch.cuda.device(self.device):
            gdn = [None if g is None else api.GDN(g[0], g[1], inverse=g[2], shift=g[3]) for g in self.gdn_np]
        self.main = api.RaggedNet(self.sizes, params=main_params, device=self.device, gdn=gdn if use_gdn else None, rgb_layout=rgb_layout)
        self.ha_np, self.hs_np = hp["ha_np"], hp["hs_np"]
        lat = self.main.shapes(3)                                           # [(h, w, 192)]
        self.h_a = api.RaggedNet([(w, h) for h, w, _ in lat], params=list(hp["pa"]), device=self.device, descs=hp["da"])
        hyp = self.h_a.shapes(1)                                            # [(h, w, 128)]
        self.h_s = api.RaggedNet([(w, h) for h, w, _ in hyp], params=list(hp["ps"]), device=self.device, descs=hp["ds"])
        self.crop = api.RaggedCrop([(h, w) for h, w, _ in self.h_s.shapes(1)], [(h, w) for h, w, _ in lat], lat[0][2], device=self.device)
        # the stream length of z: codec.auto_stream_symbols of EACH image's own hyper-latent, HyperpriorCodec's rule
        self.z_coder = codec.RaggedLatentCoder([(h, w) for h, w, _ in hyp], hyp[0][2], self.sizes, stream_symbols=z_stream_symbols or "auto",
                                               device=self.device)
        # the stream length of y: None = 16384 (auto_stream_symbols is not applied), one value, or one per image
        self.y_coder = codec.RaggedContextCoder([(h, w) for h, w, _ in lat], lat[0][2], self.sizes, stream_symbols=y_stream_symbols,
                                                device=self.device)
        u8 = dict(dtype=torch.uint8, device=self.device)
        self.y = torch.empty(self.main.nbytes(3), **u8)
        self.z = torch.empty(self.h_a.nbytes(1), **u8)
        self.z_hat = torch.empty_like(self.z)
        self.s_full = torch.empty(self.h_s.nbytes(1), **u8)
        self.s = torch.empty_like(self.y)
        self.y_hat = torch.empty_like(self.y)
        for net in (self.main, self.h_a, self.h_s):
            net.workspace()
        self._external = None       # the device copies of decode()'s external containers: alive until the next decode
        # what an archive of this codec is tagged with: the GDN specification version (include/sicn_gdn.h) with GDN, 0 without — an
        # archive written under another version of the activation, or by the other configuration, is refused (status bit 5)
        self.use_gdn = bool(use_gdn)
        self.archive_tag = int(api._lib.lib().sicn_gdn_spec_version()) if self.use_gdn else 0
        self._archive = None        # codec.RaggedArchive over (z_coder, y_coder), made on first use
        self._unpacked = False      # the last decode read an archive: check() reports its verdict first
        self._rois = {}             # decode(rois=)'s RaggedHyperpriorRoi objects by rectangles, made on first use
        self._last_roi = None       # ... the one the last decode used: check() reads its y verdicts

    def _scale_map(self, z):
        self.h_s.run_layers(0, 1, z, out=self.s_full)
        return self.crop.run(self.s_full, self.s)

    def encode(self, packed_x):
        """packed_x: the ragged input (main.pack) -> one z and one y container per image.  Enqueue only, on the current stream."""
        self._last_roi = None                   # check() reads the y coder's own verdicts again
        self.main.run_layers(0, 3, packed_x, out=self.y)
        self.h_a.run_layers(0, 1, self.y, out=self.z)
        self.z_coder.encode(self.z)
        self._scale_map(self.z)                 # z itself: the z coder is lossless (HyperpriorCodec.encode)
        self.y_coder.encode(self.y, self.s)
        return self.z_coder.slot_buffer, self.y_coder.slots()

    def _upload(self, containers, coder, what):
        """A list of `bytes` -> (a device slot buffer of `coder`'s layout holding them, a device int32 [n][2] status {0, length})."""
        import torch
        images = coder.images[:len(self.sizes)]
        if len(containers) != len(images):
            raise ValueError(f"{what}: need {len(images)} containers")
        host = torch.zeros(coder.slot_bytes, dtype=torch.uint8)
        for i, (c, im) in enumerate(zip(containers, images)):
            if len(c) > int(im.slot_bytes):
                raise ValueError(f"{what}[{i}]: {len(c)} bytes are more than the {int(im.slot_bytes)} a container of this shape may take")
            host[int(im.slot_offset):int(im.slot_offset) + len(c)] = torch.frombuffer(bytearray(c), dtype=torch.uint8)
        return host.to(self.device), torch.tensor([[0, len(c)] for c in containers], dtype=torch.int32).to(self.device)

    def _ragged_archive(self):
        if self._archive is None:
            self._archive = codec.RaggedArchive([self.z_coder, self.y_coder], tag=self.archive_tag, device=self.device)
        return self._archive

    def archive(self):
        """The containers of the last encode as ONE byte string (codec.RaggedArchive: sections z and y, tag = the GDN specification
        version with GDN, 0 without), packed on the device; `codec.split_archive` gives `containers()`.  Synchronises; raises if the
        encode reported an error."""
        ar = self._ragged_archive()
        ar.pack()
        b = ar.bytes()
        ar.check()
        return b

    @classmethod
    def from_archive(cls, b, seed: int = 0, device="cuda", use_gdn=None, main_params=None, images=None, rgb_layout: str = "interleaved"):
        """The codec for the images an archive names — all of them, or the selection `images` (strictly ascending indices into the
        archive): sizes and the z stream lengths are READ from the z containers' headers, the y stream lengths from the y containers', and `use_gdn` (unless given) from the tag —
        0 means an archive written without GDN.  `decode(archive=b, images=images)` then reads it."""
        info = codec.archive_info(b)
        sel = range(info["n_images"]) if images is None else codec._selection(images, n_archive=info["n_images"])
        heads = [info["headers"][i][0] for i in sel]
        if info["n_sections"] != 2 or any(h is None for h in heads):
            raise ValueError("not a hyperprior archive: need the sections z and y of every image")
        return cls([info["image_sizes"][i] for i in sel], seed=seed, device=device, use_gdn=info["tag"] != 0 if use_gdn is None else use_gdn,
                   main_params=main_params, z_stream_symbols=[int(h.stream_symbols) for h in heads],
                   y_stream_symbols=[int(h[1].stream_symbols) if h[1] is not None else None for h in (info["headers"][i] for i in sel)],
                   rgb_layout=rgb_layout)

    def _decode_scales(self, z_containers=None, y_containers=None, archive=None, images=None):
        """The front half of every decode, in full: unpack (with an archive), the z coder, h_s and its crop -> self.s.  Returns the y
        section's `valid` array (an archive) or None.  ValueError before any launch for arguments that do not go together."""
        if images is not None and archive is None:
            raise ValueError("images= selects from an archive")
        self._unpacked = archive is not None
        self._external = keep = []
        y_valid = None
        if archive is not None:
            if z_containers is not None or y_containers is not None:
                raise ValueError("either an archive or lists of containers")
            z_valid, y_valid = self._ragged_archive().unpack(archive, images=images)
            self.z_coder.decode(self.z_hat, valid=z_valid)
        elif z_containers is None:
            self.z_coder.decode(self.z_hat)
        else:
            buf, status = self._upload(z_containers, self.z_coder, "z_containers")
            keep += [buf, status]
            self.z_coder.decode(self.z_hat, slots=buf, valid=status)
        self._scale_map(self.z_hat)
        return y_valid

    def roi(self, rects, roi_layout=None, direct=None):
        """A RaggedHyperpriorRoi over this codec: one pixel rectangle (x0, y0, w, h), or None, per image."""
        return RaggedHyperpriorRoi(self, rects, roi_layout=roi_layout, direct=direct)

    def moving_roi(self, slots, roi_layout=None, direct=None):
        """A MovingHyperpriorRoi over this codec: `slots` = (image, w, h) per slot, positions given per `decode` call, from device
        memory."""
        return MovingHyperpriorRoi(self, slots, roi_layout=roi_layout, direct=direct)

    def decode(self, out=None, z_containers=None, y_containers=None, archive=None, images=None, rois=None, roi_layout=None, direct=None):
        """Containers (default: the last encode's; else lists of `bytes`, one per image; or `archive`, what `archive()` returned) ->
        the reconstructions, a ragged tensor of main's boundary 7 (`main.cropped(out)` cuts them to the images' sizes; a planar main
        writes them at those sizes).  An archive is
        unpacked on the device into the coders' own slots; one whose tag is not this codec's (another GDN specification version, or
        the other `use_gdn`) is refused as a whole: `check()` raises with bit 5.  Enqueue only.
        `images` (with `archive` only): the archive may hold more images than this codec; a strictly ascending sequence of
        len(self.sizes) indices into it names the ones to decode (ValueError otherwise, before any launch).
        `rois`: one (x0, y0, w, h) per image, or None for that image whole — `roi(rois).decode(...)` in one call: only the y streams,
        latent columns and pixels the rectangles need are decoded, and the result is the ROI pixels as a ragged [h][w][3] tensor
        (`roi_views` gives them per image), the bytes of the full decode cut to the rectangles.  A wrong length or a rectangle outside
        its image is a ValueError before any launch.  `roi_layout`, `direct` (with `rois`): as in RaggedHyperpriorRoi."""
        if rois is not None:
            rects = tuple(None if r is None else tuple(int(v) for v in r) for r in rois)
            key = (rects,) + api._roi_options(self.main, "decode(rois=)", roi_layout, direct)
            if key not in self._rois:
                self._rois[key] = RaggedHyperpriorRoi(self, rects, roi_layout=roi_layout, direct=direct)
            self._last_roi = self._rois[key]
            return self._last_roi.decode(archive=archive, images=images, z_containers=z_containers, y_containers=y_containers, out=out)
        self._last_roi = None
        y_valid = self._decode_scales(z_containers, y_containers, archive, images)
        if archive is not None:
            self.y_coder.decode(self.y_hat, self.s, valid=y_valid)
        elif y_containers is None:
            self.y_coder.decode(self.y_hat, self.s)
        else:
            buf, status = self._upload(y_containers, self.y_coder, "y_containers")
            self._external += [buf, status]
            self.y_coder.decode(self.y_hat, self.s, slots=buf, valid=status)
        out, _ = self.main.run_layers(4, 7, self.y_hat, out=out)
        return out

    def roi_views(self, roi_pixels):
        """Per-image [h][w][3] views of what the last `decode(rois=...)` returned."""
        if self._last_roi is None:
            raise ValueError("decode(rois=...) has not run")
        return self._last_roi.views(roi_pixels)

    def containers(self):
        """[(z container, y container)] of the last encode as `bytes` (synchronises; raises if the encode reported an error)."""
        return list(zip(self.z_coder.containers(), self.y_coder.containers()))

    def check(self):
        """Raises SicnError if the last encode / decode reported an error (synchronises); a y coder's error names its image
        (`.image` of the exception, and in its text); a refused archive raises first, with its bits (`.bits`)."""
        if self._unpacked:
            self._archive.check()
        self.z_coder.check()
        try:
            (self._last_roi.window if self._last_roi is not None else self.y_coder).check()
        except api._lib.SicnError as e:
            err = api._lib.SicnError(e.code, f"image {e.image} {self.sizes[e.image]}: {e}")
            err.image = e.image
            raise err from None

    def bytes_per_image(self):
        return [a + b for a, b in zip(self.z_coder.sizes(), self.y_coder.sizes())]


class RaggedHyperpriorRoi:
    """One pixel rectangle of every image of a RaggedHyperpriorCodec's batch, decoded without the rest of the image's y streams,
    latent columns and pixels (include/sicn_ragged_ctx_window.h).  The chain of `decode`:

        z coder, h_s and its crop   in FULL: z has 1/16 of y's positions and h_s ends at latent resolution, while layers 4-7 make
                                    256 pixels per latent position; a windowed h_s is out of scope
        codec.RaggedContextWindowDecoder   the y streams of both checkerboard sets that hold the latent rows, with the halo the
                                    class rule asks for -> the band tensor (seven enqueued operations)
        api.RaggedCut               the latent columns out of every band
        api.RaggedNet 4 .. 7        a net made for the windows' sizes (16 cw, 16 rh) on `codec.main`'s weights, descs and GDN objects
        api.RaggedCut               the rectangle out of every reconstruction -> the ROI pixels, a ragged [h][w][3] tensor

    Same bytes as `codec.decode` + `main.cropped`, sliced.  rects: one (x0, y0, w, h) per image, or None for that image whole;
    ValueError before anything is made for a wrong length or a rectangle outside its image.  Also `codec.roi(rects)` and, in one
    call, `codec.decode(..., rois=rects)`.
    roi_layout, direct: see `api._roi_options`.  With `direct`, layer 7 of the window net stores the rectangles itself — [h][w][3]
    or, planar, [3][h][w] per image — and the last cut is gone; `pixel_cut` is None."""

    def __init__(self, codec_, rects, roi_layout=None, direct=None):
        self.roi_layout, self.direct = api._roi_options(codec_.main, "RaggedHyperpriorRoi", roi_layout, direct)
        n = len(codec_.sizes)
        if len(rects) != n:
            raise ValueError(f"rects: one per image, {n}")
        self.codec = codec_
        net = codec_.main
        self.rects = [(0, 0, w, h) if r is None else tuple(int(v) for v in r) for r, (w, h) in zip(rects, codec_.sizes)]
        self.plans = [api.roi_plan(size, r) for size, r in zip(codec_.sizes, self.rects)]     # ValueError before anything is made
        self.window = codec_.y_coder.window([(p["r0"], p["rh"]) for p in self.plans])
        self.latent_cut, self.window_net, self.pixel_cut = api._roi_chain(
            net, self.plans, self.rects, [(int(im.band_rows), int(im.band_offset)) for im in self.window.images[:n]],
            [p["r0"] - int(im.band_row0) for p, im in zip(self.plans, self.window.images)], self.roi_layout, self.direct)
        self.status = self.window.status

    def decode(self, archive=None, images=None, z_containers=None, y_containers=None, out=None):
        """Containers as in `RaggedHyperpriorCodec.decode` (default: the last encode's) -> the ROI pixels, a ragged [h][w][3]
        tensor.  Enqueue only; `check()` raises for what the archive, the z coder or the window decoder reported."""
        import torch
        c = self.codec
        c._last_roi = self
        y_valid = c._decode_scales(z_containers, y_containers, archive, images)
        self.band = torch.empty(self.window.band_bytes, dtype=torch.uint8, device=c.device)
        if archive is not None:
            self.window.decode(self.band, c.s, valid=y_valid)
        elif y_containers is None:
            self.window.decode(self.band, c.s)
        else:
            buf, status = c._upload(y_containers, c.y_coder, "y_containers")
            c._external += [buf, status]
            self.window.decode(self.band, c.s, slots=buf, valid=status)
        self.latent = self.latent_cut.run(self.band)
        if self.direct:
            return self.window_net.run_layers(4, len(c.main.descs) - 1, self.latent, out=out)[0]
        recon, _ = self.window_net.run_layers(4, len(c.main.descs) - 1, self.latent)
        return self.pixel_cut.run(recon, out)

    def views(self, roi):
        """Per-image [h][w][3] views of what `decode` returned ([3][h][w] with roi_layout="planar")."""
        if self.direct:
            return self.window_net.views(len(self.codec.main.descs) - 1, roi)
        return self.pixel_cut.views(roi)

    def check(self):
        """The codec's `check()` in its order — archive, z, then y with the image named — with this object's window as the y decoder."""
        self.codec._last_roi = self
        self.codec.check()


class MovingHyperpriorRoi(api._MovingRoiChain):
    """Pixel rectangles of fixed SIZE whose POSITIONS are read from device memory on every call, decoded from a
    RaggedHyperpriorCodec's containers (include/sicn_ragged_ctx_roi_move.h).  Made once for a list of slots; what does not depend on
    a rectangle runs once per set of containers, in `prepare`:

        unpack (an archive), the z coder, h_s and its crop   codec._decode_scales -> codec.s, the FULL scale maps
        parse, tables, scan of the y containers' fixed part  three launches over the images the slots name

    and `decode(xy)` then costs its own enqueued operations and nothing else — no allocation, no upload, no host synchronisation:

        placement, band memset, anchor streams, non-anchor streams, verdicts, latent cut   six (five without non-anchor capacity)
        api.RaggedNet 4 .. 7    a net made for the sizes (16 cw_cap, 16 rh_cap) on `codec.main`'s weights, descs and GDN objects
        the pixel cut           one

    fourteen with GDN, eleven without.  Same bytes as `codec.decode` + `main.cropped`, sliced.  slots: (image, w, h) per slot, `image`
    an index into the codec's batch; several slots may name one image, in any order.  A position outside [0, image - size] is
    clamped and bit 0 of the slot's `.flags` word says so.  `.status`: device int32 [n_slots][2], the verdicts per slot;
    `.flags`: device int32 [n_slots].  The containers must stay the bytes `prepare` read until the last `decode` of them has run.
    Also `codec.moving_roi(slots)`."""
    _free, _abi, _slot_type, _n_totals = "sicn_ragged_ctx_roi_move_free", "sicn_ragged_ctx_roi_move", api._lib.RaggedCtxRoiMoveSlot, 7

    def __init__(self, codec_, slots, roi_layout=None, direct=None):
        self.codec = codec_
        self._check_slots(codec_.main, slots, roi_layout, direct)
        self._make(codec_.main, codec_.y_coder)
        self._containers = None     # (slot buffer, valid or None) of the last prepare: kept alive, read by every decode
        self._unpacked = False      # the last prepare read an archive: check() reports its verdict first

    def prepare(self, archive=None, images=None, z_containers=None, y_containers=None):
        """Containers as in `RaggedHyperpriorCodec.decode` (default: the last encode's): everything of a decode that no rectangle
        changes — unpack, the z coder, h_s and its crop (-> codec.s), and the y containers' fixed part.  Enqueue only, on the current
        stream; once per set of containers, then any number of `decode`s."""
        c = self.codec
        y = c.y_coder
        y_valid = c._decode_scales(z_containers, y_containers, archive, images)
        self._unpacked = archive is not None
        if archive is not None:
            buf, valid = y.slot_buffer, y_valid
        elif y_containers is None:
            buf, valid = y.slot_buffer, y.enc_status
        else:
            buf, valid = c._upload(y_containers, y, "y_containers")
        self._containers = (buf, valid)
        api._lib.check(api._lib.lib().sicn_ragged_ctx_roi_move_prepare_async(
            self._h, ctypes.c_void_p(buf.data_ptr()), None if valid is None else ctypes.c_void_p(valid.data_ptr()),
            ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(), api._stream_ptr(None)), "sicn_ragged_ctx_roi_move_prepare_async")

    def decode(self, xy, out=None, stream=None):
        """xy: the positions (x0, y0) per slot — a contiguous CUDA int32 tensor [n_slots][2], read when the kernels run, or a host
        sequence, which is copied into the object's own device tensor on the stream.  Returns the ROI pixels: `out` (a flat tensor
        of roi_bytes; default the object's own), as [n_slots][h][w][3] where all slots have one size, flat otherwise (`views` gives
        them per slot).  Enqueue only, nothing allocated.  RuntimeError if `prepare` has not run."""
        if self._containers is None:
            raise RuntimeError("prepare() has not run: there is no container whose fixed part a decode could read")
        return self._decode(self._positions(xy, stream), out, stream, ctypes.c_void_p(self._containers[0].data_ptr()),
                            ctypes.c_void_p(self.codec.s.data_ptr()))

    def place(self, xy):
        """Host arithmetic (sicn_ragged_ctx_roi_move_place): per slot the dict {x0, y0 after the clamp, c0, r0, cw, rh, x, y, flags,
        first_stream, end_stream (per set), band_row0, band_rows, symbols, lat_bias, cut_offset}."""
        _lib = api._lib
        y, out = self.codec.y_coder, []
        for (img, w, h), s, (x0, y0) in zip(self.slots, self.layout, xy):
            (lh, lw), (iw, ih) = y.shapes[img], self.codec.sizes[img]
            p = _lib.RaggedCtxRoiPlaced()
            _lib.check(_lib.lib().sicn_ragged_ctx_roi_move_place(iw, ih, lw, lh, y.lat_c, int(y.stream_symbols[img]), w, h, int(x0), int(y0),
                                                                 int(s.band_offset), ctypes.byref(p)), "sicn_ragged_ctx_roi_move_place")
            d = {k: int(getattr(p.px, k)) for k, _ in _lib.RaggedRoiPlaced._fields_}
            d.update(first_stream=tuple(p.first_stream), end_stream=tuple(p.end_stream), band_row0=int(p.band_row0),
                     band_rows=int(p.band_rows), symbols=int(p.symbols), lat_bias=int(p.lat_bias), cut_offset=int(p.cut_offset))
            out.append(d)
        return out

    def check(self):
        """Synchronises and raises SicnError for what the last `prepare` and `decode` reported: the archive first (`.bits`), then
        the z coder, then the slots' verdicts — the exception's `.slot` and `.image` name the first slot that failed."""
        import torch
        c = self.codec
        if self._unpacked:
            c._archive.check()
        c.z_coder.check()
        torch.cuda.synchronize(self.device)
        d = self.status[:, 0].cpu().tolist()
        if any(d):
            k = next(i for i, v in enumerate(d) if v)
            img = self.slots[k][0]
            err = api._lib.SicnError(-22, f"slot {k}, image {img} {c.sizes[img]}: moving ROI decode status {d}")
            err.slot, err.image = k, img
            raise err
