"""CPU tests of the annotated-video feature: clasfv_render_annotated's argument checks (they precede any HIP
call, so they need no GPU), the header against the ctypes signature, render.py's own checks, and
tests/render_oracle.py against the reference-run fixture tests/golden/overlay.npz and against the other reading
of nearest-neighbour resizing."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import render_oracle as R
from tests.conftest import REPO, golden

HEADER = os.path.join(REPO, "include", "clasfv.h")
EINVAL, EBADSHAPE = -1, -2
ORDER = ["video", "masks", "truth", "t", "h", "w", "volume", "vstride", "title", "first", "count", "hp", "wo", "ht", "hs",
         "label", "thickness", "work", "out", "stream"]


def test_render_refusals_need_no_gpu():
    """Null required pointers, sizes below 1 (Ht, Hs below 0), count < 1, frames outside [0, T), a label outside
    [0, 255], a negative or non-finite thickness, a stride below 1, misaligned doubles and an output that overlaps
    any input or the workspace are refused with CLASFV_EINVAL and a message; an output of 2^32 bytes or more, or
    a source of 2^31 pixels, with CLASFV_EBADSHAPE -- before any HIP call (the pointers are never dereferenced)."""
    from clasfv_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    M = 1 << 30  # the fake buffers are 1 GiB apart
    ok = dict(video=P(1 * M), masks=P(2 * M), truth=P(3 * M), t=6, h=5, w=9, volume=P(4 * M), vstride=1, title=P(5 * M),
              first=0, count=6, hp=20, wo=11, ht=3, hs=4, label=1, thickness=2.0, work=P(6 * M), out=P(7 * M), stream=None)
    inf, nan = float("inf"), float("nan")
    thw, total = 6 * 5 * 9, 6 * 27 * 11 * 3
    bad = [dict(video=None), dict(masks=None), dict(volume=None), dict(work=None), dict(out=None),
           dict(t=0), dict(h=0), dict(w=0), dict(hp=0), dict(wo=0), dict(h=-1), dict(ht=-1), dict(hs=-1),
           dict(count=0), dict(count=-1), dict(first=-1), dict(first=6, count=1), dict(first=1, count=6),
           dict(first=5, count=2), dict(first=2 ** 31 - 1, count=2 ** 31 - 1),
           dict(label=-1), dict(label=256), dict(thickness=-0.5), dict(thickness=inf), dict(thickness=nan),
           dict(vstride=0), dict(vstride=-12), dict(volume=P(4 * M + 4)), dict(work=P(6 * M + 1)),
           # out over the last byte of each input, and each input over the last byte of out
           dict(out=P(1 * M + 12 * thw - 1)), dict(out=P(2 * M + thw - 1)), dict(out=P(3 * M + thw - 1)),
           dict(out=P(4 * M + 8 * 6 - 1)), dict(out=P(4 * M + 8 * (5 * 12 + 1) - 1), vstride=12),
           dict(out=P(5 * M + 3 * 11 * 3 - 1)), dict(out=P(6 * M + 15)),
           dict(video=P(7 * M + total - 1)), dict(masks=P(7 * M + total - 1)), dict(truth=P(7 * M + total - 1)),
           dict(title=P(7 * M + total - 1)), dict(out=P(2 * M - total + 1))]
    for change in bad:
        a = dict(ok, **change)
        assert lib.clasfv_render_annotated(*[a[k] for k in ORDER]) == EINVAL, change
        assert lib.clasfv_last_error(), change
    far = dict(video=P(1 << 40), masks=P(2 << 40), truth=None, volume=P(3 << 40), title=None, work=P(4 << 40),
               out=P(5 << 40))
    for change in (dict(t=86, count=86, hp=4096, wo=4096, ht=0, hs=0),           # 86 * 3 * 2^24 >= 2^32
                   dict(t=1000, count=1000, hp=2000, wo=1000), dict(hp=2 ** 31 - 1, wo=2 ** 31 - 1, count=1),
                   dict(hp=1, ht=2 ** 31 - 1, hs=2 ** 31 - 1, wo=1, count=1), dict(h=65536, w=32768),
                   dict(h=2 ** 31 - 1, w=2 ** 31 - 1, t=2 ** 31 - 1, count=1)):
        a = dict(ok, **far, **change)
        assert lib.clasfv_render_annotated(*[a[k] for k in ORDER]) == EBADSHAPE, change
        assert lib.clasfv_last_error(), change
    assert lib.clasfv_render_workspace_bytes() == 16


def test_header_and_binding_agree():
    """The declaration of clasfv_render_annotated in the header has the ctypes signature's parameters, in order."""
    from clasfv_amd import _lib
    txt = open(HEADER).read()
    m = re.search(r"^int clasfv_render_annotated\((.*?)\);", txt, re.M | re.S)
    assert m, "clasfv_render_annotated is not declared in include/clasfv.h"
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    want = []
    for param in m.group(1).split(","):
        param = " ".join(param.split())
        want.append(ctypes.c_void_p if "*" in param else kinds[param.rsplit(" ", 1)[0]])
    res, args = _lib.SIGNATURES["clasfv_render_annotated"]
    assert res is ctypes.c_int and args == want and len(args) == len(ORDER)
    assert re.search(r"^int64_t clasfv_render_workspace_bytes\(void\);", txt, re.M)
    assert _lib.SIGNATURES["clasfv_render_workspace_bytes"] == (ctypes.c_int64, [])
    assert "#define CLASFV_ABI_VERSION 3" in txt  # new exports only
    assert "floor(255 * clip(x, 0, 1))" in txt and "not to a cv2 build" in txt  # the two rules the header must state


def test_annotate_video_python_checks_need_no_gpu():
    """render.annotate_video raises ValueError before the library is called: arrays, CPU tensors, wrong shapes
    and dtypes, labels, sizes, frame ranges, thickness."""
    from clasfv_amd import render
    video = torch.zeros((3, 4, 6, 8))
    masks = torch.zeros((4, 6, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="on the GPU"):
        render.annotate_video(video, masks)
    with pytest.raises(ValueError, match="tensor"):
        render.annotate_video(video.numpy(), masks)
    with pytest.raises(ValueError, match="tensor"):
        render.annotate_video(video, masks.numpy())
    for v, m, kw, why in ((video[0], masks, {}, "video"), (video.double(), masks, {}, "video"),
                          (video[:2], masks, {}, "video"), (video[:, :0], masks[:0], {}, "video"),
                          (video, masks[:3], {}, "masks"), (video, masks.float(), {}, "integer dtype"),
                          (video, masks, dict(truth=masks[:, :5]), "truth"),
                          (video, masks, dict(truth=masks.double()), "integer dtype"),
                          (video, masks, dict(label=256), "label"), (video, masks, dict(label=-1), "label"),
                          (video, masks, dict(label=1.5), "label"), (video, masks, dict(size=0), "size"),
                          (video, masks, dict(size=7.5), "size"), (video, masks, dict(pane_height=0), "pane_height"),
                          (video, masks, dict(title_height=-1), "title_height"),
                          (video, masks, dict(strip_height=-1), "strip_height"),
                          (video, masks, dict(first=-1), "frames"), (video, masks, dict(first=4), "frames"),
                          (video, masks, dict(count=0), "frames"), (video, masks, dict(first=2, count=3), "frames"),
                          (video, masks, dict(thickness=-1.0), "thickness"),
                          (video, masks, dict(thickness=float("nan")), "thickness"),
                          (video, masks, dict(size=40000, pane_height=40000), "addresses")):
        with pytest.raises(ValueError, match=why):
            render.annotate_video(v, m, **kw)
    with pytest.raises(ValueError, match="frames"):
        render.write_gif(np.zeros((4, 5, 3), np.uint8), "unused.gif")


def test_title_band_is_cached_and_sized():
    from clasfv_amd import render
    band = render.title_band(40, 553)
    assert band.shape == (40, 553, 3) and band.dtype == np.uint8 and render.title_band(40, 553) is band
    flat = band.reshape(-1, 3).astype(int)  # shades of lime on black (the built-in font may be anti-aliased)
    assert (flat[:, 0] == flat[:, 2]).all() and (flat[:, 1] >= flat[:, 0]).all() and (flat[:, 1] <= 205).all()
    assert render.title_band(0, 9).shape == (0, 9, 3) and render.title_band(3, 2).shape == (3, 2, 3)
    assert (render.SIZE, render.TITLE_HEIGHT, render.STRIP_HEIGHT) == (553, 40, 80)


def test_oracle_pane_equals_the_reference_fixture():
    """tests/render_oracle.py against echonet_overlay run by the reference (overlay.npz): floor(255 * ref),
    exactly, for the overlay and for the difference image. A pixel is fragile when 255 * ref is within 1e-9 of
    an integer while ref is neither 0 nor 1; the fixture has none, and has pixels clipped at both ends."""
    d, g = R.overlay_inputs(), golden("overlay.npz")
    for key, truth in (("overlay", None), ("diff", d["gt"])):
        ref = g[key]
        assert ref.dtype == np.float64 and ref.shape == (4, 24, 40, 3)
        y = 255.0 * ref
        fragile = (np.abs(y - np.round(y)) < 1e-9) & (ref != 0) & (ref != 1)
        assert int(fragile.sum()) == 0
        assert (ref == 0).sum() > 100 and (ref == 1).sum() > 100
        assert np.array_equal(R.pane_source(d["video"], d["seg"], 1, truth), np.floor(y).astype(np.uint8)), key
    assert (d["seg"] == 2).any() and ((d["seg"] == 1) & (d["gt"] != 1)).any() and ((d["seg"] != 1) & (d["gt"] == 1)).any()


def test_nearest_rule_equals_integer_reading_at_the_tested_sizes():
    """min(floor(x * (1.0 / (dst / src))), src - 1) equals (x * src) // dst at every column of the sizes the GPU
    tests and the CLI use, so neither reading of INTER_NEAREST is in doubt there."""
    for src, dst in ((112, 553), (16, 553), (24, 40), (7, 20), (9, 11), (24, 10), (40, 17), (5, 33), (9, 33), (7, 30)):
        assert np.array_equal(R.nearest_index(dst, src), (np.arange(dst) * src) // dst), (src, dst)


def test_oracle_strip_by_hand():
    """The strip rule on curves whose picture is known: frame 0 and a video without a finite volume are black; a
    constant curve is one horizontal bar of the thickness around the middle row, ending at the frame's sample;
    a NaN removes the two segments it ends."""
    T, Hs, Wo = 9, 10, 20  # S = 0.5: two columns per sample
    const = np.full(T, 5.0)
    assert not R.strip(const, 0, Hs, Wo, 2.0).any()
    assert not R.strip(np.full(T, np.nan), T - 1, Hs, Wo, 2.0).any()
    assert not R.strip(np.r_[np.nan, 1.0, np.full(T - 2, np.nan)], T - 1, Hs, Wo, 2.0).any()  # no finite pair
    s = R.strip(const, 4, Hs, Wo, 2.0)[..., 1] > 0
    # y = (105 - 5) * 10 / 200 = 5; the rows [r, r + 1) meeting [4, 6] are 4, 5 and 6 (row 6 at its top edge, row 3
    # not: it ends before 4); the columns that reach a segment before sample 4 are x = 0..7 (column 8 starts at it)
    assert s[:, :8].all(axis=1).tolist() == [r in (4, 5, 6) for r in range(Hs)] and not s[:, 8:].any()
    assert (R.strip(const, 4, Hs, Wo, 0.0)[..., 1] > 0)[:, 0].tolist() == [r == 5 for r in range(Hs)]
    gap = const.copy()
    gap[2] = np.nan  # segments 1-2 and 2-3 vanish: samples [1, 3] = columns 2..5
    s = R.strip(gap, 8, Hs, Wo, 2.0)[..., 1] > 0
    assert s.any(axis=0).tolist() == [x < 2 or 6 <= x <= 15 for x in range(Wo)]
    assert set(map(tuple, R.strip(const, 8, Hs, Wo, 2.0).reshape(-1, 3))) == {(0, 0, 0), (50, 205, 50)}
