"""Latent container ("SICL" v1) + static rANS coder on the GPU — Python wrapper of include/sicn_codec.h.

EXTENSION BEYOND THE REFERENCE: the reference has no coder, so nothing here
mirrors a reference interface and parity is "unpinned" (own specification: oracle/sicn_codec_oracle.c)."""
from __future__ import annotations

import ctypes
import numbers

from . import _lib

RAW8, PACKED7, RANS, RANSW, RANSWC = 0, 1, 2, 3, 4
__all__ = ["RAW8", "PACKED7", "RANS", "RANSW", "RANSWC", "encode_latent", "decode_latent", "parse_header", "encode_latents",
           "decode_latents", "LatentCoder", "RaggedLatentCoder", "RaggedWindowDecoder", "ContextCoder", "RaggedContextCoder", "RaggedContextWindowDecoder",
           "auto_stream_symbols", "WSTREAM_SYMBOLS",
           "RaggedArchive", "split_archive", "archive_info", "subset_archive"]


WSTREAM_SYMBOLS = 16384   # SICN_CODEC_WSTREAM_SYMBOLS: the default (and longest) rANS-W stream


def auto_stream_symbols(n_symbols: int, n_images: int = 1) -> int:
    """Stream length of the rANS-W coder as a function of ONE image's latent only (`n_images` is accepted and ignored: the
    bitstream of an image must not depend on how many images were coded beside it — ADVICE r3; a container written by a batch of
    8 decodes in a batch of 1).  A stream is a serial chain on one wave and ends with 260 bytes of flush (its 64 final states and
    its length entry), so the choice trades latency against bytes:
      * 16384 (the format's default, 2.8 % flush at 4.5 bit / symbol) for latents of at least 128 such streams — a 4K image's
        6.2 M symbols are 380;
      * 8192 otherwise (one 1080p latent: 192 streams, half the chain, + 2.8 % bytes: 3.54 instead of 3.45 bit / pixel).
    Shorter streams remain an explicit choice (`stream_symbols=2048`: a quarter of that chain again, + 14 % bytes)."""
    del n_images
    return 16384 if n_symbols >= 128 * 16384 else 8192


def _stream_ptr(stream):
    import torch
    stream = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(getattr(stream, "cuda_stream", stream))


def _valid_ptr(own_status, own: bool, valid):
    """The `valid` argument of a decode as the library takes it.  None — the whole slot is trusted — for `valid=False` and, by
    default, for slots that are not the object's own; by default the object's encoder status (`own_status`) for its own slots;
    otherwise the status array the caller passed."""
    if valid is False or (valid is None and not own):
        return None
    return ctypes.c_void_p((own_status if valid is None else valid).data_ptr())


def encode_latent(latent, image_width: int, image_height: int, mode: int = RANSW, stream=None):
    """latent: CUDA uint8 tensor [H/16][W/16][C] (one image).  Returns a CUDA uint8 tensor holding the container."""
    import torch
    L = _lib.lib()
    if not (latent.is_cuda and latent.dtype == torch.uint8 and latent.is_contiguous() and latent.dim() == 3):
        raise TypeError("latent must be a contiguous CUDA uint8 tensor [h][w][c]")
    h, w, c = (int(v) for v in latent.shape)
    n = h * w * c
    out = torch.empty(max(L.sicn_codec_max_bytes(mode, n), 64), dtype=torch.uint8, device=latent.device)
    ws = torch.empty(max(L.sicn_codec_workspace_bytes(mode, n), 64), dtype=torch.uint8, device=latent.device)
    nbytes = ctypes.c_size_t(0)
    _lib.check(L.sicn_codec_encode(mode, ctypes.c_void_p(latent.data_ptr()), w, h, c, image_width, image_height,
                                   ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.byref(nbytes),
                                   ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream_ptr(stream)), "sicn_codec_encode")
    return out[: nbytes.value]


def parse_header(container_bytes: bytes) -> "_lib.CodecInfo":
    info = _lib.CodecInfo()
    buf = (ctypes.c_uint8 * len(container_bytes)).from_buffer_copy(container_bytes)
    _lib.check(_lib.lib().sicn_codec_parse_header(buf, len(container_bytes), ctypes.byref(info)), "sicn_codec_parse_header")
    return info


def decode_latent(container, stream=None):
    """container: CUDA uint8 tensor.  Returns (latent [h][w][c] CUDA uint8, CodecInfo)."""
    import torch
    L = _lib.lib()
    info = parse_header(bytes(container[:48].cpu().numpy().tobytes()))
    n = int(info.n_symbols)
    latent = torch.empty((int(info.lat_h), int(info.lat_w), int(info.lat_c)), dtype=torch.uint8, device=container.device)
    ws = torch.empty(max(L.sicn_codec_workspace_bytes(int(info.mode), n), 64), dtype=torch.uint8, device=container.device)
    container = container.contiguous()
    _lib.check(L.sicn_codec_decode(ctypes.c_void_p(container.data_ptr()), container.numel(),
                                   ctypes.c_void_p(latent.data_ptr()), max(n, 1), ctypes.byref(info),
                                   ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream_ptr(stream)), "sicn_codec_decode")
    return latent, info


def encode_latents(latents, image_width: int, image_height: int, stream=None):
    """latents: CUDA uint8 tensor [n][H/16][W/16][C].  One rANS-W container per image, byte-identical to
    `encode_latent(latents[i], ...)`, with two host synchronisations for the whole batch.  Returns
    (slots, sizes): a CUDA uint8 tensor [n][slot_bytes] and the list of valid byte counts."""
    import torch
    L = _lib.lib()
    if not (latents.is_cuda and latents.dtype == torch.uint8 and latents.is_contiguous() and latents.dim() == 4):
        raise TypeError("latents must be a contiguous CUDA uint8 tensor [n][h][w][c]")
    nimg, h, w, c = (int(v) for v in latents.shape)
    n = h * w * c
    slot = (int(L.sicn_codec_max_bytes(RANSW, n)) + 255) // 256 * 256
    out = torch.empty((nimg, slot), dtype=torch.uint8, device=latents.device)
    ws = torch.empty(max(L.sicn_codec_batch_workspace_bytes(RANSW, n, nimg), 64), dtype=torch.uint8, device=latents.device)
    sizes = (ctypes.c_size_t * max(nimg, 1))()
    _lib.check(L.sicn_codec_encode_batch(RANSW, ctypes.c_void_p(latents.data_ptr()), nimg, w, h, c, image_width, image_height,
                                         ctypes.c_void_p(out.data_ptr()), slot, sizes, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                         _stream_ptr(stream)), "sicn_codec_encode_batch")
    return out, [int(sizes[i]) for i in range(nimg)]


def decode_latents(slots, sizes, stream=None):
    """Inverse of `encode_latents`: (slots [n][slot_bytes], sizes) -> (latents [n][h][w][c], [CodecInfo])."""
    import torch
    L = _lib.lib()
    nimg, slot = (int(v) for v in slots.shape)
    info0 = parse_header(bytes(slots[0, :48].cpu().numpy().tobytes()))
    n = int(info0.n_symbols)
    latents = torch.empty((nimg, int(info0.lat_h), int(info0.lat_w), int(info0.lat_c)), dtype=torch.uint8, device=slots.device)
    ws = torch.empty(max(L.sicn_codec_batch_workspace_bytes_sl(n, nimg, int(info0.stream_symbols)), 64), dtype=torch.uint8, device=slots.device)
    csz = (ctypes.c_size_t * nimg)(*sizes)
    infos = (_lib.CodecInfo * nimg)()
    slots = slots.contiguous()
    _lib.check(L.sicn_codec_decode_batch(ctypes.c_void_p(slots.data_ptr()), slot, csz, nimg, ctypes.c_void_p(latents.data_ptr()),
                                         max(n, 1), infos, ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream_ptr(stream)),
               "sicn_codec_decode_batch")
    return latents, list(infos)


class LatentCoder:
    """The asynchronous rANS-W batch pair (sicn_codec_encode_batch_async / sicn_codec_decode_batch_async) with its
    buffers allocated once: n latents of one shape per call, nothing but kernel launches on the current stream — no
    host synchronisation, so analysis -> encode -> decode -> synthesis can be enqueued back to back (or captured in
    one hipGraph).  Verdicts and sizes stay on the device until `check()` / `sizes()` fetch them."""

    def __init__(self, n_images: int, lat_h: int, lat_w: int, lat_c: int, image_width: int = 0, image_height: int = 0,
                 device="cuda", stream_symbols=None):
        """stream_symbols: None or "auto" = `auto_stream_symbols` of ONE image's latent (16384 for large latents, 8192 below 2 M
        symbols), or a power of two 1024 .. 16384 (sicn_codec_*_async_sl: shorter streams = shorter critical path on small latents,
        260 bytes per extra stream).  A decoder object must be built with the encoder's value — the container header carries it:
        `LatentCoder.for_containers(slots, n)` builds the matching decoder for containers made elsewhere (e.g. by the C entry points
        without `_sl`, which always write 16384-symbol streams, or by another stream length on the encoder's side)."""
        import torch
        L = _lib.lib()
        self.shape = (int(n_images), int(lat_h), int(lat_w), int(lat_c))
        self.image_wh = (int(image_width), int(image_height))
        n = lat_h * lat_w * lat_c
        self.stream_symbols = auto_stream_symbols(n) if stream_symbols in (None, "auto") else int(stream_symbols)
        if self.stream_symbols not in (1024, 2048, 4096, 8192, 16384):
            raise ValueError("stream_symbols must be a power of two in 1024 .. 16384")
        self.slot = (int(L.sicn_codec_max_bytes_sl(n, self.stream_symbols)) + 255) // 256 * 256
        dev = torch.device(device)
        self.slots = torch.empty((n_images, self.slot), dtype=torch.uint8, device=dev)
        self.ws = torch.empty(max(L.sicn_codec_batch_workspace_bytes_sl(n, n_images, self.stream_symbols), 256), dtype=torch.uint8, device=dev)
        self.enc_status = torch.zeros((n_images, 2), dtype=torch.int32, device=dev)   # sicn_codec_status {error, bytes}
        self.dec_status = torch.zeros((n_images, 2), dtype=torch.int32, device=dev)

    @classmethod
    def for_containers(cls, slots, device=None):
        """A decoder for n rANS-W containers that came from somewhere else: shape and stream length are READ from the first
        container's 48-byte header (sicn_codec_parse_header), so a default-constructed LatentCoder — whose stream length is the
        per-image automatic one — is never pointed at containers of another length (the decode would report status bit 2).
        slots: CUDA uint8 [n][slot_bytes].  One small device-to-host copy (the header), once."""
        info = parse_header(bytes(slots[0, :48].cpu().numpy().tobytes()))
        if int(info.mode) != RANSW:
            raise ValueError(f"container mode {int(info.mode)} is not rANS-W")
        coder = cls(int(slots.shape[0]), int(info.lat_h), int(info.lat_w), int(info.lat_c), int(info.image_width), int(info.image_height),
                    device=device if device is not None else slots.device, stream_symbols=int(info.stream_symbols))
        if int(slots.shape[1]) < coder.slot:   # the writer sized its slots for its own stream length; ours can only be equal or smaller
            raise ValueError(f"slots of {int(slots.shape[1])} bytes are shorter than the {coder.slot} bytes a container of this shape may take")
        if int(slots.shape[1]) != coder.slot:   # this object's own container buffer follows the slot size it is told to use: an encode()
            import torch                         # through it must never write past a buffer sized for the smaller slot
            coder.slot = int(slots.shape[1])
            coder.slots = torch.empty((coder.shape[0], coder.slot), dtype=torch.uint8, device=coder.slots.device)
        return coder

    def encode(self, latents, stream=None):
        """latents: CUDA uint8 [n][h][w][c] -> self.slots (containers), self.enc_status. Enqueue only."""
        import torch
        if not (latents.is_cuda and latents.dtype == torch.uint8 and latents.is_contiguous() and tuple(latents.shape) == self.shape):
            raise TypeError(f"latents must be a contiguous CUDA uint8 tensor of shape {self.shape}")
        n, h, w, c = self.shape
        _lib.check(_lib.lib().sicn_codec_encode_batch_async_sl(
            ctypes.c_void_p(latents.data_ptr()), n, w, h, c, self.image_wh[0], self.image_wh[1],
            ctypes.c_void_p(self.slots.data_ptr()), self.slot, ctypes.c_void_p(self.enc_status.data_ptr()),
            ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(), _stream_ptr(stream), self.stream_symbols), "sicn_codec_encode_batch_async_sl")
        return self.slots

    def decode(self, out_latents, slots=None, valid=None, stream=None):
        """slots (default: self.slots) -> out_latents [n][h][w][c], self.dec_status. `valid`: device int32 [n][2] status
        array whose `.bytes` bound each slot.  Default: this object's own encoder status when it decodes its OWN slots; with
        external `slots` the whole slot is trusted (the header's payload field is validated anyway) unless the caller passes
        the status array that travelled with them.  Pass False to trust the whole slot in every case. Enqueue only."""
        import torch
        n, h, w, c = self.shape
        slots = self.slots if slots is None else slots
        if not (out_latents.is_cuda and out_latents.dtype == torch.uint8 and out_latents.is_contiguous() and tuple(out_latents.shape) == self.shape):
            raise TypeError(f"out_latents must be a contiguous CUDA uint8 tensor of shape {self.shape}")
        if not (slots.is_cuda and slots.dtype == torch.uint8 and slots.is_contiguous() and tuple(slots.shape) == (n, self.slot)):
            raise TypeError("slots must be a contiguous CUDA uint8 tensor [n][slot_bytes]")
        vptr = _valid_ptr(self.enc_status, slots is self.slots, valid)
        _lib.check(_lib.lib().sicn_codec_decode_batch_async_sl(
            ctypes.c_void_p(slots.data_ptr()), self.slot, vptr, n, w, h, c, ctypes.c_void_p(out_latents.data_ptr()), h * w * c,
            ctypes.c_void_p(self.dec_status.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(), _stream_ptr(stream),
            self.stream_symbols), "sicn_codec_decode_batch_async_sl")
        return out_latents

    def sizes(self):
        """Container sizes of the last encode (synchronises)."""
        return [int(v) for v in self.enc_status[:, 1].cpu().tolist()]

    def check(self):
        """Raises SicnError if the last encode / decode reported an error (synchronises)."""
        e = self.enc_status[:, 0].cpu().tolist()
        d = self.dec_status[:, 0].cpu().tolist()
        if any(e):
            raise _lib.SicnError(-22, f"rANS-W encode status {e}")
        if any(d):
            raise _lib.SicnError(-22 if any(v & ~128 for v in d) else -74, f"rANS-W decode status {d}")


class _RaggedCoder(_lib.Handle):
    """What RaggedLatentCoder and RaggedContextCoder share: the arrays that describe the batch, layout and library object, the slot
    buffer, the workspace and the two status tensors; `for_containers`, the per-image views and `containers`.  A subclass names its
    entry points (`_layout`, `_create`, `_workspace_bytes`, `_free`), the struct of its layout (`_image_type`), its container mode
    and display name (`_mode`, `_name`), whether its errors carry `.image`, and how it resolves `stream_symbols`; `encode` and
    `decode` are the subclass's own."""
    _layout = _create = _workspace_bytes = ""
    _image_type, _mode, _name, _error_image = None, None, "", False

    def __init__(self, shapes, lat_c: int, image_sizes=None, stream_symbols=None, device=None):
        import torch
        L = _lib.lib()
        self.shapes = [(int(h), int(w)) for h, w in shapes]
        self.lat_c = int(lat_c)
        n = len(self.shapes)
        self.image_sizes = [(int(w), int(h)) for w, h in image_sizes] if image_sizes is not None else [(0, 0)] * n
        if len(self.image_sizes) != n:
            raise ValueError("image_sizes: one (width, height) per shape")
        self.stream_symbols = self._stream_symbols(stream_symbols)
        u32 = ctypes.c_uint32 * max(n, 1)
        self._lat_w, self._lat_h = u32(*[w for _, w in self.shapes]), u32(*[h for h, _ in self.shapes])
        self._wss = u32(*self.stream_symbols)
        self._img_w, self._img_h = u32(*[w for w, _ in self.image_sizes]), u32(*[h for _, h in self.image_sizes])
        self.images = (self._image_type * max(n, 1))()               # where image i lies: offsets, slot capacity, its streams
        totals = (ctypes.c_uint64 * 3)()
        _lib.check(getattr(L, self._layout)(self._lat_w, self._lat_h, self.lat_c, self._wss, n, self.images, totals), self._layout)
        self.latent_bytes, self.slot_bytes = int(totals[0]), int(totals[1])
        self.device = torch.device(device if device is not None else "cuda")
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(getattr(L, self._create)(self._lat_w, self._lat_h, self.lat_c, self._wss, self._img_w, self._img_h, n,
                                                ctypes.byref(self._h)), self._create)
        self.slot_buffer = torch.empty(self.slot_bytes, dtype=torch.uint8, device=self.device)
        self.ws = torch.empty(max(int(getattr(L, self._workspace_bytes)(self._h)), 256), dtype=torch.uint8, device=self.device)
        self.enc_status = torch.zeros((n, 2), dtype=torch.int32, device=self.device)   # sicn_codec_status {error, bytes}
        self.dec_status = torch.zeros((n, 2), dtype=torch.int32, device=self.device)

    @classmethod
    def for_containers(cls, containers, device=None):
        """A coder for containers of this coder's mode that came from somewhere else (a list of `bytes`): shapes, image sizes and
        stream lengths are READ from the 48-byte headers, the containers are copied into the coder's slots and their lengths into
        its encoder status, so that `decode` reads exactly them."""
        import torch
        infos = [parse_header(bytes(c[:48])) for c in containers]
        if not infos:
            raise ValueError("no containers")
        if any(int(i.mode) != cls._mode for i in infos) or len({int(i.lat_c) for i in infos}) != 1:
            raise ValueError(f"containers must all be {cls._name} and of one channel count")
        coder = cls([(int(i.lat_h), int(i.lat_w)) for i in infos], int(infos[0].lat_c),
                    [(int(i.image_width), int(i.image_height)) for i in infos], [int(i.stream_symbols) for i in infos], device=device)
        host = torch.zeros(coder.slot_bytes, dtype=torch.uint8)
        for c, im in zip(containers, coder.images):
            if len(c) > int(im.slot_bytes):
                raise ValueError(f"a container of {len(c)} bytes is longer than the {int(im.slot_bytes)} its shape may take")
            host[int(im.slot_offset):int(im.slot_offset) + len(c)] = torch.frombuffer(bytearray(c), dtype=torch.uint8)
        coder.slot_buffer.copy_(host)
        coder.enc_status.copy_(torch.tensor([[0, len(c)] for c in containers], dtype=torch.int32))
        return coder

    def slots(self, slot_buffer=None):
        """Per-image views of the slot buffer (default: this object's own), each the slot's whole capacity."""
        buf = self.slot_buffer if slot_buffer is None else slot_buffer
        return [buf[int(im.slot_offset):int(im.slot_offset) + int(im.slot_bytes)] for im in self.images[:len(self.shapes)]]

    def views(self, latents):
        """Per-image [h][w][c] views of a ragged latent tensor."""
        return [latents[int(im.latent_offset):int(im.latent_offset) + h * w * self.lat_c].view(h, w, self.lat_c)
                for im, (h, w) in zip(self.images, self.shapes)]

    def _flat(self, t, nbytes, what):
        import torch
        if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == (nbytes,)):
            raise TypeError(f"{what} must be a contiguous CUDA uint8 tensor of {nbytes} bytes")

    def _error(self, code, what, status):
        """The SicnError of a status column with a set word; with `_error_image`, `.image` is the first image that failed."""
        err = _lib.SicnError(code, f"{self._name} {what} status {status}")
        if self._error_image:
            err.image = next(i for i, v in enumerate(status) if v)
        return err

    sizes = LatentCoder.sizes

    def containers(self):
        """The containers of the last encode as `bytes`, one per image (synchronises; raises if the encode reported an error)."""
        import torch
        torch.cuda.synchronize(self.device)
        status = self.enc_status.cpu().tolist()
        if any(e for e, _ in status):
            raise self._error(-22, "encode", [e for e, _ in status])
        host = self.slot_buffer.cpu().numpy()
        return [host[int(im.slot_offset):int(im.slot_offset) + size].tobytes() for im, (_, size) in zip(self.images, status)]


class _RaggedWindow(_lib.Handle):
    """What the two window decoders share: the checks of `rows`, the arrays, layout and library object, `status` and `check`.  A
    subclass names its entry points (`_layout`, `_create`, `_free`) and the struct of its layout (`_image_type`); `selected_streams`,
    `views` and `decode` are its own, because the band layouts differ."""
    _layout = _create = ""
    _image_type = None

    def __init__(self, coder, rows):
        import torch
        L = _lib.lib()
        self.coder = coder              # keeps the coder (and its device tables) alive
        n = len(coder.shapes)
        self.rows = [(int(r0), int(rh)) for r0, rh in rows]
        if len(self.rows) != n:
            raise ValueError("rows: one (r0, rh) per image of the coder")
        if any(r0 < 0 or rh < 1 or r0 + rh > h for (r0, rh), (h, _) in zip(self.rows, coder.shapes)):
            raise ValueError("a window of latent rows must be non-empty and lie inside its latent")
        u32 = ctypes.c_uint32 * max(n, 1)
        self._r0, self._rh = u32(*[r for r, _ in self.rows]), u32(*[h for _, h in self.rows])
        self.images = (self._image_type * max(n, 1))()
        totals = (ctypes.c_uint64 * 2)()
        _lib.check(getattr(L, self._layout)(coder._lat_w, coder._lat_h, coder.lat_c, coder._wss, self._r0, self._rh, n, self.images, totals),
                   self._layout)
        self.band_bytes = int(totals[0])
        self._h = ctypes.c_void_p()
        with torch.cuda.device(coder.device):
            _lib.check(getattr(L, self._create)(coder._h, self._r0, self._rh, ctypes.byref(self._h)), self._create)
        self.status = torch.zeros((n, 2), dtype=torch.int32, device=coder.device)

    def check(self):
        """Synchronises and raises if a window reported an error (an rANS-WC window's exception carries `.image`, the first image
        that failed)."""
        import torch
        torch.cuda.synchronize(self.coder.device)
        d = self.status[:, 0].cpu().tolist()
        if any(d):
            raise self.coder._error(-22, "window decode", d)


class RaggedLatentCoder(_RaggedCoder):
    """The ragged rANS-W pair (include/sicn_ragged_codec.h): n latents of n DIFFERENT shapes -> n containers with three launches for
    the whole batch, and back with two.  `shapes`: [(lat_h, lat_w)] per image, `lat_c` channels in all of them; `image_sizes`:
    [(width, height)], header fields only.  Latents travel as a ragged tensor — a flat CUDA uint8 tensor, the images' [h][w][c]
    arrays back to back (api.RaggedNet's boundary 3) — containers in one flat slot buffer, image i's slot at `images[i].slot_offset`.
    stream_symbols: None or "auto" = `auto_stream_symbols` of EACH image's own latent, one value for all, or one per image.
    Container i is byte-identical to `LatentCoder(1, h_i, w_i, lat_c, stream_symbols=...)`'s and decodes with `decode_latent`.
    Same conventions as LatentCoder: enqueue only; verdicts and sizes stay on the device until `check()` / `sizes()` fetch them."""
    _free, _layout, _create = "sicn_ragged_coder_free", "sicn_ragged_codec_layout", "sicn_ragged_coder_create"
    _workspace_bytes, _image_type, _mode, _name = "sicn_ragged_coder_workspace_bytes", _lib.RaggedCodecImage, RANSW, "rANS-W"

    def _stream_symbols(self, stream_symbols):
        n = len(self.shapes)
        if stream_symbols in (None, "auto"):
            return [auto_stream_symbols(h * w * self.lat_c) for h, w in self.shapes]
        if isinstance(stream_symbols, int):
            return [stream_symbols] * n
        v = [int(x) for x in stream_symbols]
        if len(v) != n:
            raise ValueError("stream_symbols: one value, or one per shape")
        return v

    def encode(self, latents, stream=None):
        """latents: ragged CUDA uint8 tensor -> self.slot_buffer (containers), self.enc_status.  Enqueue only."""
        self._flat(latents, self.latent_bytes, "latents")
        _lib.check(_lib.lib().sicn_ragged_coder_encode_async(
            self._h, ctypes.c_void_p(latents.data_ptr()), ctypes.c_void_p(self.slot_buffer.data_ptr()),
            ctypes.c_void_p(self.enc_status.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(), _stream_ptr(stream)),
            "sicn_ragged_coder_encode_async")
        return self.slot_buffer

    def decode(self, out_latents, slots=None, valid=None, stream=None):
        """slots (a flat slot buffer; default: this object's own) -> out_latents (ragged), self.dec_status.  `valid` as in
        LatentCoder.decode: default this object's encoder status for its OWN slots, the whole slot for external ones; a device
        int32 [n][2] status array, or False to trust the whole slot.  Enqueue only."""
        slots = self.slot_buffer if slots is None else slots
        self._flat(out_latents, self.latent_bytes, "out_latents")
        self._flat(slots, self.slot_bytes, "slots")
        _lib.check(_lib.lib().sicn_ragged_coder_decode_async(
            self._h, ctypes.c_void_p(slots.data_ptr()), _valid_ptr(self.enc_status, slots is self.slot_buffer, valid),
            ctypes.c_void_p(out_latents.data_ptr()), ctypes.c_void_p(self.dec_status.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()),
            self.ws.numel(), _stream_ptr(stream)), "sicn_ragged_coder_decode_async")
        return out_latents

    check = LatentCoder.check

    def window(self, rows):
        """A RaggedWindowDecoder over this coder's slots: `rows` = [(r0, rh)] per image, the latent rows [r0, r0 + rh) to decode."""
        return RaggedWindowDecoder(self, rows)


class RaggedWindowDecoder(_RaggedWindow):
    """A window of latent ROWS of every image decoded from its streams alone (include/sicn_ragged_window.h): two launches for the
    batch.  Made by `RaggedLatentCoder.window(rows)`; shapes, stream lengths, slot buffer and workspace are the coder's, so whatever
    fills the coder's slots (`encode`, `RaggedArchive.unpack`) feeds this decoder.  The result is the BAND tensor: per image the
    symbols of the streams that hold the rows, image i at `images[i].band_offset`, row r0 `images[i].lead` bytes further.
    `.status`: device int32 [n][2], the window decoder's verdicts (bit 7, the checksum of the whole latent, is never set)."""
    _free, _layout, _create = "sicn_ragged_window_free", "sicn_ragged_window_layout", "sicn_ragged_window_create"
    _image_type = _lib.RaggedWindowImage

    def __init__(self, coder, rows):
        super().__init__(coder, rows)
        self.selected_streams = sum(int(im.end_stream) - int(im.first_stream) for im in self.images[:len(self.rows)])

    def views(self, band):
        """Per-image [rh][lat_w][lat_c] views of the rows asked for, inside a band tensor (no copy)."""
        out = []
        for im, (_, rh), (_, w) in zip(self.images, self.rows, self.coder.shapes):
            at = int(im.band_offset) + int(im.lead)
            out.append(band[at:at + rh * w * self.coder.lat_c].view(rh, w, self.coder.lat_c))
        return out

    def decode(self, band, slots=None, valid=None, stream=None):
        """slots (default: the coder's own) -> band, self.status.  `valid` as in RaggedLatentCoder.decode.  Enqueue only."""
        c = self.coder
        slots = c.slot_buffer if slots is None else slots
        c._flat(band, self.band_bytes, "band")
        c._flat(slots, c.slot_bytes, "slots")
        _lib.check(_lib.lib().sicn_ragged_window_decode_async(
            self._h, ctypes.c_void_p(slots.data_ptr()), _valid_ptr(c.enc_status, slots is c.slot_buffer, valid),
            ctypes.c_void_p(band.data_ptr()), ctypes.c_void_p(self.status.data_ptr()), ctypes.c_void_p(c.ws.data_ptr()), c.ws.numel(),
            _stream_ptr(stream)), "sicn_ragged_window_decode_async")
        return band


def _ctx_stream_symbols(stream_symbols, n):
    """The rANS-WC stream lengths of n images from None (16384), one int, or one per image; ValueError for a length that is not
    admissible, before anything is made."""
    if stream_symbols is None:
        v = [WSTREAM_SYMBOLS] * n
    elif isinstance(stream_symbols, numbers.Integral) and not isinstance(stream_symbols, bool):   # (a numpy integer from a parsed header too)
        v = [int(stream_symbols)] * n
    else:
        v = [WSTREAM_SYMBOLS if x is None else int(x) for x in stream_symbols]
        if len(v) != n:
            raise ValueError("stream_symbols: one value, or one per shape")
    if any(x not in (1024, 2048, 4096, 8192, 16384) for x in v):
        raise ValueError("stream_symbols must be a power of two in 1024 .. 16384")
    return v


class ContextCoder:
    """Container mode 4 ("rANS-WC",sicn_codec_ctx_*_async): the conditional coder of the hyperprior configuration — 16
    class tables, class from the hyper-synthesis scale map and, for the non-anchor half of a checkerboard, from the
    already decoded anchor neighbours.  Same conventions as LatentCoder (enqueue only; verdicts / sizes on the device).
    stream_symbols: the stream length the encoder writes and the decoder expects (header dword 9), a power of two in 1024 .. 16384;
    None = 16384 (`auto_stream_symbols` is NOT applied to this coder)."""

    def __init__(self, n_images: int, lat_h: int, lat_w: int, lat_c: int, image_width: int = 0, image_height: int = 0,
                 device="cuda", stream_symbols=None):
        import torch
        L = _lib.lib()
        self.shape = (int(n_images), int(lat_h), int(lat_w), int(lat_c))
        self.image_wh = (int(image_width), int(image_height))
        self.stream_symbols = _ctx_stream_symbols(stream_symbols, 1)[0]
        self.slot = (int(L.sicn_codec_ctx_max_bytes_sl(lat_w, lat_h, lat_c, self.stream_symbols)) + 255) // 256 * 256
        dev = torch.device(device)
        self.slots = torch.empty((n_images, self.slot), dtype=torch.uint8, device=dev)
        self.ws = torch.empty(max(L.sicn_codec_ctx_workspace_bytes_sl(lat_w, lat_h, lat_c, n_images, self.stream_symbols), 256),
                              dtype=torch.uint8, device=dev)
        self.enc_status = torch.zeros((n_images, 2), dtype=torch.int32, device=dev)
        self.dec_status = torch.zeros((n_images, 2), dtype=torch.int32, device=dev)

    def _check(self, t, what):
        import torch
        if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == self.shape):
            raise TypeError(f"{what} must be a contiguous CUDA uint8 tensor of shape {self.shape}")

    def encode(self, latents, scales, stream=None):
        self._check(latents, "latents")
        self._check(scales, "scales")
        n, h, w, c = self.shape
        _lib.check(_lib.lib().sicn_codec_ctx_encode_batch_async_sl(
            ctypes.c_void_p(latents.data_ptr()), ctypes.c_void_p(scales.data_ptr()), n, w, h, c, self.image_wh[0], self.image_wh[1],
            ctypes.c_void_p(self.slots.data_ptr()), self.slot, ctypes.c_void_p(self.enc_status.data_ptr()),
            ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(), _stream_ptr(stream), self.stream_symbols),
            "sicn_codec_ctx_encode_batch_async_sl")
        return self.slots

    def decode(self, out_latents, scales, slots=None, valid=None, stream=None):
        self._check(out_latents, "out_latents")
        self._check(scales, "scales")
        n, h, w, c = self.shape
        slots = self.slots if slots is None else slots
        vptr = _valid_ptr(self.enc_status, slots is self.slots, valid)   # external containers: see LatentCoder.decode
        _lib.check(_lib.lib().sicn_codec_ctx_decode_batch_async_sl(
            ctypes.c_void_p(slots.data_ptr()), self.slot, vptr, ctypes.c_void_p(scales.data_ptr()), n, w, h, c,
            ctypes.c_void_p(out_latents.data_ptr()), ctypes.c_void_p(self.dec_status.data_ptr()),
            ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(), _stream_ptr(stream), self.stream_symbols),
            "sicn_codec_ctx_decode_batch_async_sl")
        return out_latents

    sizes = LatentCoder.sizes
    check = LatentCoder.check


class RaggedContextCoder(_RaggedCoder):
    """The ragged rANS-WC pair (include/sicn_ragged_ctx.h): n latents of n DIFFERENT shapes, each with its scale map -> n mode-4
    containers with six launches for the whole batch, and back with eight.  `shapes`: [(lat_h, lat_w)] per image, `lat_c` channels
    (a multiple of 4) in all of them; `image_sizes`: [(width, height)], header fields only.  Latents and scales travel as two ragged
    tensors of one layout — flat CUDA uint8 tensors, the images' [h][w][c] arrays back to back — containers in one flat slot buffer,
    image i's slot at `images[i].slot_offset`.  Container i is byte-identical to `ContextCoder(1, h_i, w_i, lat_c)`'s and decodes
    with it.  Same conventions as RaggedLatentCoder: enqueue only; verdicts and sizes stay on the device until `check()` / `sizes()`.
    stream_symbols: None (16384), one length for all images, or one per image — `ContextCoder`'s parameter; the lengths live in the
    coder, so `decode` and `window` expect them."""
    _free, _layout, _create = "sicn_ragged_ctx_coder_free", "sicn_ragged_ctx_layout_sl", "sicn_ragged_ctx_coder_create_sl"
    _workspace_bytes, _image_type, _mode, _name = "sicn_ragged_ctx_coder_workspace_bytes", _lib.RaggedCtxImage, RANSWC, "rANS-WC"
    _error_image = True

    def _stream_symbols(self, stream_symbols):
        return _ctx_stream_symbols(stream_symbols, len(self.shapes))

    def encode(self, latents, scales, stream=None):
        """latents, scales: ragged CUDA uint8 tensors -> self.slot_buffer (containers), self.enc_status.  Enqueue only."""
        self._flat(latents, self.latent_bytes, "latents")
        self._flat(scales, self.latent_bytes, "scales")
        _lib.check(_lib.lib().sicn_ragged_ctx_encode_async(
            self._h, ctypes.c_void_p(latents.data_ptr()), ctypes.c_void_p(scales.data_ptr()), ctypes.c_void_p(self.slot_buffer.data_ptr()),
            ctypes.c_void_p(self.enc_status.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(), _stream_ptr(stream)),
            "sicn_ragged_ctx_encode_async")
        return self.slot_buffer

    def decode(self, out_latents, scales, slots=None, valid=None, stream=None):
        """slots (a flat slot buffer; default: this object's own) -> out_latents (ragged), self.dec_status.  `valid` as in
        RaggedLatentCoder.decode.  Enqueue only."""
        slots = self.slot_buffer if slots is None else slots
        self._flat(out_latents, self.latent_bytes, "out_latents")
        self._flat(scales, self.latent_bytes, "scales")
        self._flat(slots, self.slot_bytes, "slots")
        _lib.check(_lib.lib().sicn_ragged_ctx_decode_async(
            self._h, ctypes.c_void_p(slots.data_ptr()), _valid_ptr(self.enc_status, slots is self.slot_buffer, valid),
            ctypes.c_void_p(scales.data_ptr()), ctypes.c_void_p(out_latents.data_ptr()), ctypes.c_void_p(self.dec_status.data_ptr()),
            ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(), _stream_ptr(stream)), "sicn_ragged_ctx_decode_async")
        return out_latents

    def window(self, rows):
        """A RaggedContextWindowDecoder over this coder's slots: `rows` = [(r0, rh)] per image, the latent rows [r0, r0 + rh) to decode."""
        return RaggedContextWindowDecoder(self, rows)

    def check(self):
        """Raises SicnError if the last encode / decode reported an error (synchronises); the exception's `.image` is the first
        image that failed."""
        e = self.enc_status[:, 0].cpu().tolist()
        d = self.dec_status[:, 0].cpu().tolist()
        for what, st in (("encode", e), ("decode", d)):
            if any(st):
                raise self._error(-74 if what == "decode" and not any(v & ~128 for v in st) else -22, what, st)


class RaggedContextWindowDecoder(_RaggedWindow):
    """A window of latent ROWS of every image decoded from its rANS-WC streams alone (include/sicn_ragged_ctx_window.h): seven
    enqueued operations for the batch.  Made by `RaggedContextCoder.window(rows)`; shapes, slot buffer and workspace are the coder's,
    so whatever fills the coder's slots (`encode`, `RaggedArchive.unpack`) feeds this decoder.  The result is the BAND tensor: per
    image the whole latent rows [band_row0, band_row0 + band_rows) at `images[i].band_offset` — the symbols of the selected streams,
    zero where a position belongs to a stream outside the selection; the rows asked for are complete.
    `.status`: device int32 [n][2], the window decoder's verdicts (bit 7, the checksum of the whole latent, is never set)."""
    _free, _layout, _create = "sicn_ragged_ctx_window_free", "sicn_ragged_ctx_window_layout_sl", "sicn_ragged_ctx_window_create"
    _image_type = _lib.RaggedCtxWindowImage

    def __init__(self, coder, rows):
        super().__init__(coder, rows)
        self.selected_streams = sum(int(im.end_stream[s]) - int(im.first_stream[s]) for im in self.images[:len(self.rows)] for s in (0, 1))

    def views(self, band):
        """Per-image [rh][lat_w][lat_c] views of the rows asked for, inside a band tensor (no copy)."""
        out = []
        for im, (r0, rh), (_, w) in zip(self.images, self.rows, self.coder.shapes):
            row = w * self.coder.lat_c
            at = int(im.band_offset) + (r0 - int(im.band_row0)) * row
            out.append(band[at:at + rh * row].view(rh, w, self.coder.lat_c))
        return out

    def decode(self, band, scales, slots=None, valid=None, stream=None):
        """slots (default: the coder's own) and the FULL scale maps (ragged, the coder's latent layout) -> band, self.status.
        `valid` as in RaggedLatentCoder.decode.  Enqueue only."""
        c = self.coder
        slots = c.slot_buffer if slots is None else slots
        c._flat(band, self.band_bytes, "band")
        c._flat(scales, c.latent_bytes, "scales")
        c._flat(slots, c.slot_bytes, "slots")
        _lib.check(_lib.lib().sicn_ragged_ctx_window_decode_async(
            self._h, ctypes.c_void_p(slots.data_ptr()), _valid_ptr(c.enc_status, slots is c.slot_buffer, valid),
            ctypes.c_void_p(scales.data_ptr()), ctypes.c_void_p(band.data_ptr()), ctypes.c_void_p(self.status.data_ptr()),
            ctypes.c_void_p(c.ws.data_ptr()), c.ws.numel(), _stream_ptr(stream)), "sicn_ragged_ctx_window_decode_async")
        return band


def _parse_archive(b):
    """(RaggedArchiveInfo, sizes, offsets) of an archive held as `bytes` — sicn_ragged_archive_parse, host only.  The library reads
    the caller's bytes in place: nothing is copied."""
    L = _lib.lib()
    if not isinstance(b, bytes):
        b = bytes(b)
    info = _lib.RaggedArchiveInfo()
    _lib.check(L.sicn_ragged_archive_parse(b, len(b), ctypes.byref(info), None, None), "sicn_ragged_archive_parse")   # the counts
    entries = int(info.n_images) * int(info.n_sections)
    sizes, offsets = (ctypes.c_uint32 * entries)(), (ctypes.c_uint64 * entries)()
    _lib.check(L.sicn_ragged_archive_parse(b, len(b), ctypes.byref(info), sizes, offsets), "sicn_ragged_archive_parse")
    return info, list(sizes), list(offsets)


def _split(b, info, sizes, offsets):
    k = int(info.n_sections)
    return [tuple(b[offsets[i * k + s]:offsets[i * k + s] + sizes[i * k + s]] for s in range(k)) for i in range(int(info.n_images))]


def split_archive(b):
    """An archive ("SICA", include/sicn_ragged_archive.h) -> per image, a tuple of its containers as `bytes`, one per section.
    Host only; raises SicnError for a malformed archive."""
    if not isinstance(b, bytes):
        b = bytes(b)
    return _split(b, *_parse_archive(b))


def archive_info(b):
    """What an archive says of itself: {"n_images", "n_sections", "tag", "total_bytes", "image_sizes": [(width, height)],
    "latent_shapes": [per image, a tuple of (lat_h, lat_w, lat_c) per section], "headers": the CodecInfo of every container}.
    Sizes and shapes are READ from each container's 48-byte header (an empty container gives None).  Host only; the archive is
    parsed once."""
    if not isinstance(b, bytes):
        b = bytes(b)
    info, sizes, offsets = _parse_archive(b)
    k = int(info.n_sections)
    headers = [tuple(parse_header(b[offsets[i * k + s]:offsets[i * k + s] + 48]) if sizes[i * k + s] else None for s in range(k))
               for i in range(int(info.n_images))]
    first = [next((h for h in hs if h is not None), None) for hs in headers]
    return {"n_images": int(info.n_images), "n_sections": int(info.n_sections), "tag": int(info.tag), "total_bytes": int(info.total_bytes),
            "image_sizes": [None if h is None else (int(h.image_width), int(h.image_height)) for h in first],
            "latent_shapes": [tuple(None if h is None else (int(h.lat_h), int(h.lat_w), int(h.lat_c)) for h in hs) for hs in headers],
            "headers": headers}


def _selection(images, n_archive=None, n_expected=None):
    """`images` as a list of ints after the checks every caller makes before any launch: strictly ascending, each in [0, n_archive),
    `n_expected` of them.  ValueError otherwise."""
    sel = [int(i) for i in images]
    if not sel:
        raise ValueError("images: an empty selection")
    if n_expected is not None and len(sel) != n_expected:
        raise ValueError(f"images: {len(sel)} indices for {n_expected} images")
    if sel[0] < 0 or any(b <= a for a, b in zip(sel, sel[1:])):
        raise ValueError("images: the indices must be strictly ascending and not negative")
    if sel[-1] >= (1 << 32 if n_archive is None else n_archive):
        raise ValueError(f"images: index {sel[-1]} is beyond the archive's {n_archive} images" if n_archive is not None else "images: index beyond 2^32")
    return sel


def subset_archive(b, images):
    """The archive of the selected images alone (sicn_ragged_archive_subset): same tag and sections, the containers copied byte for
    byte.  `images`: strictly ascending indices into the archive.  Host only; SicnError for a malformed archive."""
    L = _lib.lib()
    if not isinstance(b, bytes):
        b = bytes(b)
    sel = _selection(images)
    index = (ctypes.c_uint32 * len(sel))(*sel)
    need = ctypes.c_uint64(0)
    _lib.check(L.sicn_ragged_archive_subset(b, len(b), index, len(sel), None, 0, ctypes.byref(need)), "sicn_ragged_archive_subset")
    out = ctypes.create_string_buffer(int(need.value))
    _lib.check(L.sicn_ragged_archive_subset(b, len(b), index, len(sel), out, int(need.value), ctypes.byref(need)), "sicn_ragged_archive_subset")
    return out.raw


class RaggedArchive(_lib.Handle):
    """The containers of a ragged batch as ONE byte string (include/sicn_ragged_archive.h): packed on the device from the slot buffers
    and encoder status arrays of one to four ragged coder objects of one batch as they lie — two launches, whatever the number of
    images — and unpacked into those coders' own slot buffers with the `valid` arrays their `decode(..., valid=...)` takes, with two.
    `coders`: RaggedLatentCoder / RaggedContextCoder objects (anything with `images[i].slot_offset / .slot_bytes`, `shapes`,
    `slot_buffer` and `enc_status`), one section each, in the archive's section order.  `tag`: stored by pack, compared by unpack.
    Same conventions as the coders: pack / unpack enqueue only; `bytes()` and `check()` synchronise."""
    _free = "sicn_ragged_archive_free"

    def __init__(self, coders, tag: int = 0, device=None):
        import torch
        L = _lib.lib()
        self.coders = list(coders)
        k = len(self.coders)
        n = len(self.coders[0].shapes) if self.coders else 0
        if not 1 <= k <= 4 or any(len(c.shapes) != n for c in self.coders):
            raise ValueError("one to four coders of one batch")
        self.n_images, self.n_sections, self.tag = n, k, int(tag) & 0xFFFFFFFF
        u64 = ctypes.c_uint64 * max(n, 1)
        self._off = [u64(*[int(im.slot_offset) for im in c.images[:n]]) for c in self.coders]
        self._cap = [u64(*[int(im.slot_bytes) for im in c.images[:n]]) for c in self.coders]
        pp = ctypes.POINTER(ctypes.c_uint64) * k
        self.device = torch.device(device if device is not None else self.coders[0].device)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.sicn_ragged_archive_create(n, k, pp(*[ctypes.cast(a, ctypes.POINTER(ctypes.c_uint64)) for a in self._off]),
                                                    pp(*[ctypes.cast(a, ctypes.POINTER(ctypes.c_uint64)) for a in self._cap]),
                                                    ctypes.byref(self._h)), "sicn_ragged_archive_create")
        self.max_bytes = int(L.sicn_ragged_archive_max_bytes(self._h))
        self.ws = torch.empty(max(int(L.sicn_ragged_archive_workspace_bytes(self._h)), 256), dtype=torch.uint8, device=self.device)
        self.status = torch.zeros(4, dtype=torch.int32, device=self.device)        # sicn_ragged_archive_status {error, first_bad, bytes}
        self.buffer = None          # pack()'s device buffer of max_bytes, made on first use
        self.valid = [torch.zeros((n, 2), dtype=torch.int32, device=self.device) for _ in range(k)]   # unpack()'s {error, bytes} per section
        self._in = None             # the device copy of unpack()'s archive: alive until the next unpack
        self._index = None          # ... and of its selection (unpack(images=...))

    def _ptrs(self, tensors):
        return (ctypes.c_void_p * self.n_sections)(*[t.data_ptr() for t in tensors])

    def pack(self, stream=None, out=None):
        """The coders' slot buffers and encoder statuses -> `out` (default: this object's own buffer of `max_bytes`), self.status.
        Enqueue only."""
        import torch
        if out is None:
            if self.buffer is None:
                self.buffer = torch.empty(self.max_bytes, dtype=torch.uint8, device=self.device)
            out = self.buffer
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 1):
            raise TypeError("out must be a contiguous flat CUDA uint8 tensor")
        self._out = out
        _lib.check(_lib.lib().sicn_ragged_archive_pack_async(
            self._h, self._ptrs([c.slot_buffer for c in self.coders]), self._ptrs([c.enc_status for c in self.coders]), self.tag,
            ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.c_void_p(self.status.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()),
            self.ws.numel(), _stream_ptr(stream)), "sicn_ragged_archive_pack_async")
        return out

    def read_status(self):
        """(error bits, first_bad, bytes) of the last pack / unpack (synchronises)."""
        import torch
        torch.cuda.synchronize(self.device)
        e, bad, lo, hi = (int(v) & 0xFFFFFFFF for v in self.status.cpu().tolist())
        return e, bad, lo | hi << 32

    def check(self):
        """Raises SicnError if the last pack / unpack reported an error (synchronises); the exception carries `.bits`, and `.first_bad`
        (an entry, image * n_sections + section, or None) with `.image`."""
        e, bad, _ = self.read_status()
        if e:
            err = _lib.SicnError(-28 if e == 4 else -22, f"ragged archive status bits {e:#x}, first bad entry {None if bad == 0xFFFFFFFF else bad}")
            err.bits = e
            err.first_bad = None if bad == 0xFFFFFFFF else bad
            err.image = None if err.first_bad is None else err.first_bad // self.n_sections
            raise err

    def bytes(self):
        """The archive of the last pack as `bytes`: exactly status.bytes travel to the host (synchronises; raises on bit 2)."""
        e, _, nbytes = self.read_status()
        if e & 4:
            raise _lib.SicnError(-28, f"ragged archive: the output buffer is smaller than the {nbytes} bytes of the archive")
        return self._out[:nbytes].cpu().numpy().tobytes()

    def unpack(self, archive, stream=None, images=None):
        """`archive` (`bytes`, or a flat CUDA uint8 tensor) -> the coders' own slot buffers; returns the `valid` arrays (device int32
        [n][2], one per coder) to hand to `decode(..., valid=...)`.  A refused archive writes no slot byte and gives {error, 0} in every
        entry, so the decoders report bit 8 per image; `check()` names the archive's own verdict.  Enqueue only.
        `images`: the archive may hold MORE images than this object; container images[j] goes to slot j
        (sicn_ragged_archive_unpack_select_async).  A strictly ascending sequence of `n_images` indices into the archive — ValueError
        otherwise, before any launch — uploaded and kept alive like the archive; or a CUDA int32 tensor of `n_images` indices, taken
        as it lies and read when the kernels run (under capture, a replay reads what it holds then): the device checks it, bit 8."""
        import torch
        index = None
        if isinstance(images, torch.Tensor):
            if not (images.is_cuda and images.dtype == torch.int32 and images.is_contiguous() and tuple(images.shape) == (self.n_images,)):
                raise TypeError(f"images as a tensor: a contiguous CUDA int32 tensor of {self.n_images} indices")
            index = images
        elif images is not None:
            import numpy as np
            sel = _selection(images, n_expected=self.n_images)
            index = torch.from_numpy(np.asarray(sel, dtype=np.uint32).view(np.int32)).to(self.device)
        if not isinstance(archive, torch.Tensor):
            host = torch.frombuffer(bytearray(archive), dtype=torch.uint8) if len(archive) else torch.empty(0, dtype=torch.uint8)
            n_in = host.numel()
            archive = torch.empty(max(n_in, 16), dtype=torch.uint8, device=self.device)
            archive[:n_in].copy_(host)
        else:
            n_in = archive.numel()
            if not (archive.is_cuda and archive.dtype == torch.uint8 and archive.is_contiguous() and archive.dim() == 1):
                raise TypeError("archive must be bytes or a contiguous flat CUDA uint8 tensor")
        self._in, self._index = archive, index
        if index is None:
            _lib.check(_lib.lib().sicn_ragged_archive_unpack_async(
                self._h, ctypes.c_void_p(archive.data_ptr()), n_in, self.tag, self._ptrs([c.slot_buffer for c in self.coders]),
                self._ptrs(self.valid), ctypes.c_void_p(self.status.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(),
                _stream_ptr(stream)), "sicn_ragged_archive_unpack_async")
        else:
            _lib.check(_lib.lib().sicn_ragged_archive_unpack_select_async(
                self._h, ctypes.c_void_p(archive.data_ptr()), n_in, self.tag, ctypes.c_void_p(index.data_ptr()),
                self._ptrs([c.slot_buffer for c in self.coders]), self._ptrs(self.valid), ctypes.c_void_p(self.status.data_ptr()),
                ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(), _stream_ptr(stream)), "sicn_ragged_archive_unpack_select_async")
        return list(self.valid)
