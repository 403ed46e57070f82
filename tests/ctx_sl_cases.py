"""The reference and the inputs of tests/test_ctx_stream_length.py and tests/test_ctx_stream_length_gpu.py (no tests here).

tests/cpp/ctx_sl_reference.c — mode 4 with the stream length S a parameter, in plain C — is built into a temporary directory together
with oracle/sicn_codec_oracle.c (whose normalisation and Adler-32 it calls) and loaded with ctypes.  Every latent the tests use comes
from `latent()`, and every reference container from `container()`: computed once per (shape, S), shared, never modified.
"""
import atexit
import ctypes
import functools
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
LENGTHS = (1024, 2048, 4096, 8192, 16384)
HEADER, TABLES = 48, 16 * 256
V_HEADER, V_TABLES, V_PAYLOAD, V_STREAM, V_SUM, V_CHECKSUM, V_SHORT = 4, 8, 16, 32, 64, 128, 0x104


def cap(S):
    """Bytes a stream of S symbols can have at most: a 16-bit word per symbol and the 64 final states."""
    return 2 * S + 256


def geometry(h, w, c, S):
    """((anchor symbols, non-anchor symbols), (anchor streams, non-anchor streams)), from the checkerboard itself."""
    py, px = np.mgrid[0:h, 0:w]
    na = int(((px + py) % 2 == 0).sum()) * c
    nsym = (na, h * w * c - na)
    return nsym, tuple(-(-n // S) for n in nsym)


def max_bytes(h, w, c, S):
    _, nst = geometry(h, w, c, S)
    return HEADER + TABLES + 4 * sum(nst) + 2 * h * w * c + 256 * sum(nst)


@functools.lru_cache(maxsize=None)
def ref():
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no host C compiler for tests/cpp/ctx_sl_reference.c")
    tmp = Path(tempfile.mkdtemp(prefix="ctx_sl_ref_"))
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    so = tmp / "libctx_sl_reference.so"
    subprocess.run([cc, "-O2", "-std=c99", "-Wall", "-shared", "-fPIC", str(ROOT / "tests" / "cpp" / "ctx_sl_reference.c"),
                    str(ROOT / "oracle" / "sicn_codec_oracle.c"), "-o", str(so)], check=True, capture_output=True, text=True)
    L = ctypes.CDLL(str(so))
    p, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.ctxsl_max_bytes.argtypes = [u32] * 4
    L.ctxsl_max_bytes.restype = ctypes.c_uint64
    L.ctxsl_streams.argtypes = [u32] * 4
    L.ctxsl_streams.restype = ctypes.c_uint64
    L.ctxsl_set_streams.argtypes = [ctypes.c_int] + [u32] * 4
    L.ctxsl_set_streams.restype = ctypes.c_uint64
    L.ctxsl_encode.argtypes = [p, p] + [u32] * 6 + [p, ctypes.c_size_t]
    L.ctxsl_encode.restype = ctypes.c_longlong
    L.ctxsl_decode.argtypes = [p, ctypes.c_size_t, p] + [u32] * 4 + [p]
    L.ctxsl_decode.restype = ctypes.c_longlong
    return L


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def ref_encode(y, s, S, image_wh=(0, 0)):
    y, s = np.ascontiguousarray(y, np.uint8), np.ascontiguousarray(s, np.uint8)
    h, w, c = y.shape
    out = np.zeros(int(ref().ctxsl_max_bytes(w, h, c, S)) + 64, np.uint8)
    n = ref().ctxsl_encode(_ptr(y), _ptr(s), w, h, c, S, image_wh[0], image_wh[1], _ptr(out), out.size)
    if n < 0:
        raise RuntimeError(f"ctxsl_encode rc={n}")
    return out[:n].tobytes()


def ref_decode(blob, s, S):
    """(symbols decoded or minus the verdict class, latent) — the decoder is told shape and length, as the library's is."""
    s = np.ascontiguousarray(s, np.uint8)
    h, w, c = s.shape
    buf = np.frombuffer(bytes(blob) + b"\0" * 8, np.uint8).copy()
    lat = np.full(s.shape, 0xEE, np.uint8)
    n = ref().ctxsl_decode(_ptr(buf), len(blob), _ptr(s), w, h, c, S, _ptr(lat))
    return int(n), lat


def image_wh(shape):
    return (shape[1] * 16, shape[0] * 16)


@functools.lru_cache(maxsize=None)
def latent(shape, variant=0):
    """(y, s) [h][w][c] of one image, seeded by the shape (and `variant`, for several images of one shape): a peaked latent (most
    symbols small, as a real y) whose spread follows the scale map, so that the classes differ and the tables are not flat.  Read-only."""
    rng = np.random.default_rng(list(shape) + [variant])
    s = rng.integers(0, 128, shape, dtype=np.uint8)
    y = np.minimum(127, (rng.exponential(1.0, shape) * (1 + s.astype(np.float64) / 6)).astype(np.int64)).astype(np.uint8)
    y.setflags(write=False)
    s.setflags(write=False)
    return y, s


@functools.lru_cache(maxsize=None)
def container(shape, S, variant=0):
    """The reference's container of latent(shape, variant) at stream length S, image size 16 x the latent's."""
    y, s = latent(shape, variant)
    return ref_encode(y, s, S, image_wh(shape))


def selected_mask(shape, S, first, end):
    """[h][w][c] bool: the symbols that the streams [first[set], end[set]) of the two sets hold."""
    h, w, c = shape
    index = np.arange(h * w * c, dtype=np.int64).reshape(shape)
    order = set_order(index)
    na = geometry(h, w, c, S)[0][0]
    pos = np.empty(h * w * c, np.int64)
    pos[order] = np.arange(order.size)
    pos = pos.reshape(shape)
    py, px = np.mgrid[0:h, 0:w]
    anchor = ((px + py) % 2 == 0)[:, :, None]
    stream = np.where(anchor, pos, pos - na) // S
    return np.where(anchor, (stream >= first[0]) & (stream < end[0]), (stream >= first[1]) & (stream < end[1]))


def fields(blob):
    """(header dwords [12], table bytes, stream lengths) of a mode-4 container."""
    head = np.frombuffer(blob[:HEADER], "<u4")
    ns = int(head[8])
    return head, blob[HEADER:HEADER + TABLES], np.frombuffer(blob[HEADER + TABLES:HEADER + TABLES + 4 * ns], "<u4")


def set_order(y):
    """The symbols of y in coding order: anchors then non-anchors, pixels in raster order inside a set, channels fastest."""
    py, px = np.mgrid[0:y.shape[0], 0:y.shape[1]]
    anchor = (px + py) % 2 == 0
    return np.concatenate([y[anchor].reshape(-1), y[~anchor].reshape(-1)])
