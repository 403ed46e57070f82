"""GPU checks of the hyperprior ROI decode (hyperprior.RaggedHyperpriorRoi, RaggedHyperpriorCodec.roi / decode(rois=); run with -m gpu
on an MI355X): a pixel rectangle of each image of a ragged hyperprior batch from the y streams, latent columns and pixels it needs.
Everything is byte equality against the codec's own full decode, cropped to the images' sizes and sliced in numpy."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = [(592, 592), (768, 640), (48, 48), (100, 36)]       # (width, height)
SEED = 7


def _centred(size, w, h):
    w, h = min(w, size[0]), min(h, size[1])
    return ((size[0] - w) // 2, (size[1] - h) // 2, w, h)


def _rects(kind):
    """One rectangle (or None) per image of SIZES."""
    if kind.startswith("pixel-"):                            # one pixel, around where a window's first row and column move
        off = int(kind[6:])
        return [(off, off, 1, 1) for _ in SIZES]
    if kind == "top-left":
        return [(0, 0, min(7, w), min(5, h)) for w, h in SIZES]
    if kind == "top-right":
        return [(w - min(7, w), 0, min(7, w), min(5, h)) for w, h in SIZES]
    if kind == "bottom-left":
        return [(0, h - min(5, h), min(7, w), min(5, h)) for w, h in SIZES]
    if kind == "bottom-right":
        return [(w - 1, h - 1, 1, 1) for w, h in SIZES]
    if kind == "whole":
        return [None for _ in SIZES]
    assert kind == "centred-256"                             # where it fits; the image whole where it does not
    return [_centred(s, 256, 256) for s in SIZES]


KINDS = ["pixel-15", "pixel-16", "pixel-17", "pixel-31", "pixel-32", "top-left", "top-right", "bottom-left", "bottom-right", "whole",
         "centred-256"]


@pytest.fixture(scope="module", params=[True, False], ids=["gdn", "relu"])
def world(request):
    """(codec, per-image [h][w][3] arrays of the full decode cropped, the containers, the archive), made once per configuration."""
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import hyperprior
    rng = np.random.default_rng(33)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in SIZES]
    rc = hyperprior.RaggedHyperpriorCodec(SIZES, seed=SEED, use_gdn=request.param)
    rc.encode(rc.main.pack([torch.from_numpy(x) for x in images]))
    full = rc.decode()
    rc.check()
    want = [v.cpu().numpy() for v in rc.main.crop_views(rc.main.cropped(full))]
    for a, (w, h) in zip(want, SIZES):
        assert a.shape == (h, w, 3)
        a.setflags(write=False)
    return rc, want, rc.containers(), rc.archive(), request.param


def _cut(want, rects):
    out = []
    for a, r in zip(want, rects):
        x0, y0, w, h = (0, 0, a.shape[1], a.shape[0]) if r is None else r
        out.append(a[y0:y0 + h, x0:x0 + w])
    return out


def _same(views, want, what):
    assert len(views) == len(want)
    for i, (v, a) in enumerate(zip(views, want)):
        assert tuple(v.shape) == a.shape, f"{what}: image {i} shape"
        assert np.array_equal(v.cpu().numpy(), a), f"{what}: image {i}"


@pytest.mark.parametrize("kind", KINDS)
def test_roi_equals_the_full_decode_sliced(world, kind):
    rc, want, containers, archive, _ = world
    rects = _rects(kind)
    cut = _cut(want, rects)
    roi = rc.roi(rects)
    assert roi is not None and len(roi.plans) == len(SIZES)
    # the codec's own slots
    out = roi.decode()
    roi.check()
    _same(roi.views(out), cut, f"{kind}: own slots")
    assert roi.status.cpu().tolist() == [[0, int(im.symbols)] for im in roi.window.images[:len(SIZES)]]
    if kind not in ("whole",):
        assert roi.window.selected_streams <= sum(int(im.anchor_streams) + int(im.nonanchor_streams) for im in rc.y_coder.images[:len(SIZES)])
    # lists of containers
    out = roi.decode(z_containers=[z for z, _ in containers], y_containers=[y for _, y in containers])
    roi.check()
    _same(roi.views(out), cut, f"{kind}: lists of containers")
    # the archive
    out = roi.decode(archive=archive)
    roi.check()
    _same(roi.views(out), cut, f"{kind}: archive")
    # the one-call form, and a full decode afterwards is still the full decode
    out = rc.decode(rois=rects)
    rc.check()
    _same(rc.roi_views(out), cut, f"{kind}: decode(rois=)")
    assert torch.equal(out, roi.decode())


def test_a_large_window_leaves_most_streams_unread(world):
    rc, _, _, _, _ = world
    roi = rc.roi([_centred(SIZES[0], 256, 256), (0, 0, 1, 1), None, None])
    total = [int(im.anchor_streams) + int(im.nonanchor_streams) for im in rc.y_coder.images[:len(SIZES)]]
    sel = [sum(int(im.end_stream[s]) - int(im.first_stream[s]) for s in (0, 1)) for im in roi.window.images[:len(SIZES)]]
    assert sel[1] < total[1] and sel[0] < total[0] and sel[2:] == total[2:], (sel, total)


def test_archive_with_a_selection_and_none_entries(world):
    rc, want, _, archive, use_gdn = world
    from simple_image_compression_network_amd import hyperprior
    sel = [1, 3]
    small = hyperprior.RaggedHyperpriorCodec.from_archive(archive, seed=SEED, images=sel)
    assert small.sizes == [SIZES[i] for i in sel] and small.use_gdn == use_gdn
    rects = [_centred(SIZES[1], 256, 256), None]
    out = small.decode(archive=archive, images=sel, rois=rects)
    small.check()
    _same(small.roi_views(out), _cut([want[i] for i in sel], rects), "selection")
    roi = small.roi(rects)
    assert torch.equal(roi.decode(archive=archive, images=sel), out)
    roi.check()
    with pytest.raises(ValueError):
        small.decode(images=sel, rois=rects)                 # images= selects from an archive
    with pytest.raises(ValueError):
        small.decode(archive=archive, images=[1], rois=rects)
    # without rois the codec still decodes in full
    full = small.decode(archive=archive, images=sel)
    small.check()
    _same(small.main.crop_views(small.main.cropped(full)), [want[i] for i in sel], "full decode of the selection")


def test_wrong_rois_are_refused_before_any_launch(world):
    rc = world[0]
    before = (rc.z_coder.dec_status.clone(), rc.y_coder.dec_status.clone())
    for bad in ([None] * 3, [None] * 5, [(0, 0, 593, 1), None, None, None], [None, None, (47, 47, 2, 1), None], [None, None, None, (0, 36, 1, 1)],
                [(0, 0, 0, 1), None, None, None], [(-1, 0, 1, 1), None, None, None]):
        with pytest.raises(ValueError):
            rc.roi(bad)
        with pytest.raises(ValueError):
            rc.decode(rois=bad)
    assert torch.equal(before[0], rc.z_coder.dec_status) and torch.equal(before[1], rc.y_coder.dec_status)


def test_damaged_containers_are_reported_in_the_codecs_order(world):
    rc, want, containers, _, _ = world
    rects = [_centred(SIZES[0], 256, 256), None, None, (15, 15, 1, 1)]
    roi = rc.roi(rects)
    zs, ys = [z for z, _ in containers], [y for _, y in containers]
    # a y container: the error names its image, the others are exact
    bad = 2
    y = bytearray(ys[bad])
    y[len(y) - 100] ^= 0x40                                   # inside the last stream's payload; image 2 is decoded whole
    out = roi.decode(z_containers=zs, y_containers=ys[:bad] + [bytes(y)] + ys[bad + 1:])
    with pytest.raises(RuntimeError) as e:
        roi.check()
    assert e.value.image == bad and f"image {bad}" in str(e.value) and "rANS-WC" in str(e.value)
    with pytest.raises(RuntimeError) as e2:
        rc.check()
    assert e2.value.image == bad
    cut = _cut(want, rects)
    for i, v in enumerate(roi.views(out)):
        if i != bad:
            assert np.array_equal(v.cpu().numpy(), cut[i]), f"neighbour {i}"
    # a z container: reported by the z coder as before, ahead of y
    z = bytearray(zs[0])
    z[len(z) - 20] ^= 0x40
    roi.decode(z_containers=[bytes(z)] + zs[1:], y_containers=ys)
    with pytest.raises(RuntimeError) as e:
        roi.check()
    assert "rANS-W decode status" in str(e.value) and not hasattr(e.value, "image")
    # and the codec is unharmed
    out = roi.decode()
    roi.check()
    _same(roi.views(out), cut, "after the damaged ones")
