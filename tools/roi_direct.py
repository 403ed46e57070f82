"""What the four ROI speed tools share for `--roi-layout` / `--direct` (include/sicn_ragged_rect.h): the arguments, the keywords they
become, and the timed `--only` run of one process that prints its time per call and a hash of the ROI pixels.

Three ways to run the same decode, each in a process of its own (profiles/ragged_rect_speed.txt):
  (a)                          the default chain: layers 4-7 into a reconstruction tensor, then the pixel cut
  (b) --direct                 layer 7 stores the rectangles itself, interleaved: the same bytes as (a)
  (c) --roi-layout planar      layer 7 stores [3][h][w] per rectangle; held against
      --permute                (a) followed by one permuted copy per rectangle, what a caller who needs CHW pays today: the same
                               bytes as (c)
"""
import hashlib
import statistics
import time


def add_arguments(ap):
    ap.add_argument("--roi-layout", choices=["interleaved", "planar"], default=None,
                    help="the layout of the ROI pixels (default: today's chain, interleaved); planar needs --only")
    ap.add_argument("--direct", action="store_true", help="layer 7 stores the rectangles itself: no reconstruction tensor, no pixel cut")
    ap.add_argument("--permute", action="store_true",
                    help="with --only and the default chain: one permuted copy [h][w][3] -> [3][h][w] per rectangle after every decode")
    ap.add_argument("--batches", type=int, default=5, help="with --only: timed batches of --calls calls (the median is reported)")


def check(ap, a):
    if (a.roi_layout == "planar" or a.permute) and not a.only:
        ap.error("--roi-layout planar and --permute need --only: the table compares interleaved bytes")
    if a.permute and (a.direct or a.roi_layout == "planar"):
        ap.error("--permute is the default chain's way to planar pixels")


def keywords(a):
    """The keywords of an ROI object for these arguments; none at all for the default chain."""
    if a.roi_layout is None and not a.direct:
        return {}
    return dict(roi_layout=a.roi_layout or "interleaved", direct=True if a.direct else None)


def label(a):
    return "permute" if a.permute else "planar" if a.roi_layout == "planar" else "direct" if a.direct else "default"


def timed_only(a, what, decode, views):
    """decode() -> the ROI pixels (enqueue only); views(pixels) -> per-rectangle views.  Runs --batches batches of --calls calls,
    each timed with the host's clock around a device that is idle at both ends, and prints one line: the way, the median time per
    call with the batches' spread, and the SHA-256 of the ROI pixels as the caller ends up holding them."""
    import torch

    def once():
        pixels = decode()
        if a.permute:
            return [v.permute(2, 0, 1).contiguous() for v in views(pixels)]
        return pixels

    once()
    ms = []
    for _ in range(a.batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            got = once()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / a.calls)
    parts = got if isinstance(got, list) else list(views(got))
    digest = hashlib.sha256(b"".join(p.contiguous().cpu().numpy().tobytes() for p in parts)).hexdigest()
    print(f"{what} way={label(a)} calls={a.calls} batches={a.batches} median_ms={statistics.median(ms):.4f} min_ms={min(ms):.4f} "
          f"max_ms={max(ms):.4f} sha256={digest}")
