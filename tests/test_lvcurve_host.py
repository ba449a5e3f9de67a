"""CPU tests of the LV curve feature: clasfv_lv_geometry's argument checks (they precede any HIP call, so they
need no GPU), the CLASFV_LV_* constants, the Python-side errors of echo.lv_curve / echo.ef_from_curve,
ed_es_pairs + ef_from_curve against compute_ef_using_putative_clips, and the share of frames the robustness
predicate of tests/lvcurve_oracle.py keeps on every set tests/test_lvcurve_gpu.py uses."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import lvcurve_oracle as O
from tests.conftest import REPO, golden, unpack_labels

HEADER = os.path.join(REPO, "include", "clasfv.h")
EINVAL, EBADSHAPE = -1, -2
NORTHSTAR = ("northstar_c1.npz", "northstar_c1_random.npz", "northstar_c1_deep.npz")


def test_lv_geometry_refusals_need_no_gpu():
    """Null pointers, F < 1, H or W < 1, a label outside [0, 255] and spacings that are not finite and positive
    are refused with CLASFV_EINVAL and a message, a frame of CLASFV_LV_MAX_PIXELS + 1 pixels with
    CLASFV_EBADSHAPE -- before any HIP call (the pointers here are never dereferenced)."""
    from clasfv_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    ok = dict(masks=P(0x10000), f=3, h=5, w=9, label=1, sy=1.0, sx=1.0, area=P(0x20000), geom=P(0x40000), stream=None)
    order = ["masks", "f", "h", "w", "label", "sy", "sx", "area", "geom", "stream"]
    inf, nan = float("inf"), float("nan")
    bad = [dict(masks=None), dict(area=None), dict(geom=None), dict(f=0), dict(f=-2), dict(h=0), dict(w=0), dict(h=-1),
           dict(label=-1), dict(label=256), dict(sy=0.0), dict(sx=0.0), dict(sy=-1.0), dict(sx=-0.5), dict(sy=inf),
           dict(sx=inf), dict(sy=nan), dict(sx=nan)]
    for change in bad:
        a = dict(ok, **change)
        assert lib.clasfv_lv_geometry(*[a[k] for k in order]) == EINVAL, change
        assert lib.clasfv_last_error(), change
    for change in (dict(h=1, w=_lib.LV_MAX_PIXELS + 1), dict(h=_lib.LV_MAX_PIXELS + 1, w=1), dict(h=404, w=404),
                   dict(h=65536, w=65536)):
        a = dict(ok, **change)
        assert lib.clasfv_lv_geometry(*[a[k] for k in order]) == EBADSHAPE, change
        assert lib.clasfv_last_error(), change


def test_lv_constants_match_header():
    from clasfv_amd import _lib
    defs = {k: int(v, 0) for k, v in re.findall(r"#define CLASFV_LV_(\w+)\s+(\w+)", open(HEADER).read())}
    assert defs == {"NPUCKS": _lib.LV_NPUCKS, "STRIDE": _lib.LV_STRIDE, "MAX_PIXELS": _lib.LV_MAX_PIXELS}
    assert _lib.LV_STRIDE == _lib.LV_NPUCKS + 2 == O.NP + 2
    assert _lib.LV_MAX_PIXELS == 160 * 1024 - 1024  # one frame's bytes and 1 KiB of state in one CU's LDS
    assert 403 * 404 <= _lib.LV_MAX_PIXELS < 404 * 404


def test_lv_curve_python_checks_need_no_gpu():
    """echo.lv_curve raises ValueError for CPU tensors, float masks, bad shapes, labels and spacings, and
    echo.ef_from_curve for curves that are not one video's -- all before the library is called."""
    from clasfv_amd import echo
    z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype)
    for masks in (z(3, 4, 6), z(2, 3, 4, 6, dtype=torch.int64)):
        with pytest.raises(ValueError, match="on the GPU"):
            echo.lv_curve(masks)
    with pytest.raises(ValueError, match="tensor"):
        echo.lv_curve(np.zeros((3, 4, 6), np.uint8))
    for masks, kw, why in ((z(3, 4, 6, dtype=torch.float32), {}, "integer dtype"),
                           (z(3, 4, 6, dtype=torch.float64), {}, "integer dtype"),
                           (z(4, 6), {}, "expected"), (z(2, 3, 4, 5, 6), {}, "expected"), (z(0, 4, 6), {}, "expected"),
                           (z(3, 0, 6), {}, "expected"), (z(1, 404, 404), {}, "pixels"),
                           (z(3, 4, 6), dict(label=256), "label"), (z(3, 4, 6), dict(label=-1), "label"),
                           (z(3, 4, 6), dict(label=1.5), "label"), (z(3, 4, 6), dict(spacing=(0.0, 1.0)), "spacing"),
                           (z(3, 4, 6), dict(spacing=(1.0, float("nan"))), "spacing"),
                           (z(3, 4, 6), dict(spacing=(1.0, float("inf"))), "spacing"),
                           (z(3, 4, 6), dict(spacing=(1.0, -2.0)), "spacing")):
        with pytest.raises(ValueError, match=why):
            echo.lv_curve(masks, **kw)
    for area, volume in ((np.zeros((2, 5)), np.zeros((2, 5))), (np.zeros(5), np.zeros(6)), (np.zeros(()), np.zeros(()))):
        with pytest.raises(ValueError):
            echo.ef_from_curve(area, volume, "x")


def _host_curve(masks):
    """(area, volume) of a 0/1 mask video by the host functions, one get2dPucks per frame."""
    from clasfv_amd import echo
    with np.errstate(invalid="ignore", divide="ignore"):
        vol = np.array([echo._disk_volume(*echo.get2dPucks((m == 1).astype(int), (1.0, 1.0))) for m in masks])
    return (masks == 1).sum(axis=(1, 2)).astype(np.int32), vol


def _ef_videos():
    for name in NORTHSTAR:
        yield name, unpack_labels(golden(name), "fused_simple")
    g = golden("ef.npz")
    for name in g["names"]:
        shp = tuple(g[name + "_shape"])
        yield str(name), np.unpackbits(g[name + "_bits"])[: int(np.prod(shp))].reshape(shp).astype(np.int64)


def test_ef_from_host_curve_reproduces_compute_ef_exactly(capsys):
    """ed_es_pairs + ef_from_curve on the per-frame host curve give the pairs and EFs of
    compute_ef_using_putative_clips bit for bit, dropped negative EFs and their message included, on the three
    northstar fixtures' fused masks and on every mask video of ef.npz."""
    from clasfv_amd import echo
    seen = 0
    for name, masks in _ef_videos():
        capsys.readouterr()
        efs, pairs = echo.compute_ef_using_putative_clips(masks, name, return_edes=True)
        said = capsys.readouterr().out
        area, vol = _host_curve(masks)
        assert echo.ed_es_pairs(area) == pairs
        got, got_pairs = echo.ef_from_curve(area, vol, name, return_edes=True)
        assert capsys.readouterr().out == said
        assert got_pairs == pairs and len(got) == len(efs)
        assert np.array_equal(np.array(got, np.float64), np.array(efs, np.float64), equal_nan=True), name
        again = echo.ef_from_curve(torch.from_numpy(area), torch.from_numpy(vol), name)  # tensors are taken too
        assert np.array_equal(np.array(again, np.float64), np.array(got, np.float64), equal_nan=True), name
        seen += len(pairs)
    assert seen >= 6


def test_robust_share_of_every_gpu_set():
    """The cap of the GPU tests, checked where no GPU is needed: the predicate keeps at least 90 % of the frames
    of every generated set, with the spacing of the spacing test too, and of the three northstar videos; the
    hand-made frames and the half-planes are robust by construction; the checkerboards tie by construction
    (their cuts fall on pixel diagonals), so the GPU test compares their area and length only."""
    with_nan = 0
    for h, w in O.SIZES:
        frames = O.oracle_frames(O.ellipse_masks(h, w))
        assert O.left_out(frames) <= O.MAX_LEFT_OUT, (h, w)
        with_nan += sum(f.robust and bool(np.isnan(f.radii).any()) for f in frames)
    assert with_nan >= 20  # the noisy masks do bring empty slabs (NaN radii) among the frames compared in full
    assert O.left_out(O.oracle_frames(O.ellipse_masks(13, 29), spacing=(0.5, 2.0))) <= O.MAX_LEFT_OUT
    for name in NORTHSTAR:
        frames = O.oracle_frames(unpack_labels(golden(name), "fused_simple"))
        assert O.left_out(frames) <= O.MAX_LEFT_OUT, name
        pairs = golden(name)["pairs_simple"].reshape(-1)
        assert all(frames[i].robust for i in pairs), name  # every ED and ES frame
    assert all(O.oracle_frame(fr == lab).robust for _, fr, lab in O.hand_frames())
    for h, w in ((112, 112), (200, 200), (403, 404)):
        assert O.oracle_frame(O.half_plane(h, w)).robust
        assert np.isfinite(O.oracle_frame(O.checkerboard(h, w)).length)
