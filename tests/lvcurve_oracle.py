"""Oracle, robustness predicate and seeded masks shared by tests/test_lvcurve_host.py and
tests/test_lvcurve_gpu.py (clasfv_lv_geometry / echo.lv_curve).

The oracle is echo.py's host code: get2dPucks and _disk_volume per frame. get2dPucks is discontinuous: a
rim pixel whose major-axis coordinate ties with a slab cut lands in one slab or the other depending on the
last ulp of LAPACK's eigenvectors, and so does the pixel next to the one attaining the maximum. No second
implementation reproduces that, so radii are compared on ROBUST frames only -- a predicate of the oracle's own
intermediate values (numpy, float64, the steps of get2dPucks), margins 1e-6, a thousand times the 1e-9 the
comparison allows."""
import warnings

import numpy as np

from clasfv_amd import echo

NP = 10
MARGIN = 1e-6   # relative margin that defines a robust frame
RTOL = 1e-9     # length, radii, volume on robust frames: float64 rounding, FMA contraction, another eigen formula
MAX_LEFT_OUT = 0.10


class Frame:
    """Oracle values of one mask frame. ``robust``: radii and volume can be compared; ``axes_ok``: length can."""
    __slots__ = ("area", "length", "radii", "volume", "robust", "axes_ok")


def oracle_frame(member, spacing=(1.0, 1.0)):
    member = np.asarray(member, bool)
    f = Frame()
    f.area = int(member.sum())
    f.robust = f.axes_ok = True
    if f.area < 2:  # get2dPucks: (1.0, zeros) for no pixel, (0.0, zeros) for one
        f.length, f.radii = echo.get2dPucks(member, spacing)
        f.length, f.volume = float(f.length), 0.0
        return f
    if member.all():  # no rim: the host function raises, the batch call gives NaN
        f.length, f.radii, f.volume = np.nan, np.full(NP, np.nan), np.nan
        return f
    with np.errstate(invalid="ignore", divide="ignore"):
        length, radii = echo.get2dPucks(member, spacing)
        f.length, f.radii, f.volume = float(length), radii, float(echo._disk_volume(length, radii))
    # get2dPucks' own steps again, for the predicate
    sp = np.asarray(spacing, np.float64).reshape(2, 1)
    pts = np.stack(np.nonzero(member)) * sp
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        cov = np.cov(pts, rowvar=True)
    if cov[0, 1] == 0.0 and cov[1, 0] == 0.0:
        return f  # (c) diagonal covariance: the axes are the coordinate axes on both sides, exactly
    evals, evecs = np.linalg.eig(cov)
    axes = evecs[:, np.argsort(evals)[::-1]]
    axes = axes * np.where(np.diag(axes) < 0, -1.0, 1.0)
    f.axes_ok = bool(abs(evals[0] - evals[1]) > MARGIN * np.max(np.abs(evals)) and
                     abs(axes[0, 0]) > MARGIN and abs(axes[1, 1]) > MARGIN)  # (a)
    rim = np.stack(np.nonzero(echo.thick_boundary(member))) * sp
    x = np.dot((rim - pts.mean(axis=1, keepdims=True)).T, axes)[:, 0]
    cuts = np.linspace(x.min(), x.max(), NP + 1)
    others = np.delete(x, np.argmax(x))
    clear = others.size == 0 or np.abs(others[:, None] - cuts[None, 1:]).min() > MARGIN * (x.max() - x.min())  # (b)
    f.robust = bool(f.axes_ok and clear)
    return f


def oracle_frames(frames, label=1, spacing=(1.0, 1.0)):
    return [oracle_frame(np.asarray(fr) == label, spacing) for fr in frames]


def left_out(frames):
    """Share of frames whose radii are not compared."""
    return sum(not f.robust for f in frames) / len(frames)


def compare(frames, area, length, radii, volume, what="", rim_count=False):
    """Area exact everywhere; on robust frames length, radii and volume within RTOL relative with the NaN
    pattern equal; on the others length when the axes are well defined. Asserts that at most MAX_LEFT_OUT of
    the frames were left out. ``rim_count``: the rim-count frames, whose FIRST frame is a checkerboard. A
    checkerboard ties with its cuts by construction, so it can never be robust; its length is compared all the
    same (the length survives the sign ambiguity of an axis that (a) guards against), and the cap is asserted
    over the other frames."""
    area, length, radii, volume = (np.asarray(a) for a in (area, length, radii, volume))
    assert area.shape == (len(frames),) and radii.shape == (len(frames), NP), what
    np.testing.assert_array_equal(area, [f.area for f in frames], err_msg=what)
    for i, f in enumerate(frames):
        msg = f"{what} frame {i}"
        if f.robust or f.axes_ok or rim_count:
            np.testing.assert_allclose(length[i], f.length, rtol=RTOL, atol=0, equal_nan=True, err_msg=msg)
        if f.robust:
            np.testing.assert_allclose(radii[i], f.radii, rtol=RTOL, atol=0, equal_nan=True, err_msg=msg)
            np.testing.assert_allclose(volume[i], f.volume, rtol=RTOL, atol=0, equal_nan=True, err_msg=msg)
    capped = frames[1:] if rim_count else frames
    assert left_out(capped) <= MAX_LEFT_OUT, f"{what}: {left_out(capped):.1%} of the frames are not robust"


SIZES = [(16, 16), (13, 29), (7, 40), (31, 17), (48, 80), (112, 112), (1, 9), (9, 1), (2, 2)]


def ellipse_masks(h, w, count=100, seed=0):
    """(count, h, w) uint8: seeded tilted ellipses with random centre, semi-axes and angle; every 4th with 3 %
    salt noise (several components: empty slabs, NaN radii), every 7th with 2 % of the pixels set to 2."""
    rng = np.random.default_rng([seed, h, w])
    ii, jj = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((count, h, w), np.uint8)
    for f in range(count):
        ci, cj = rng.uniform(0.2, 0.8) * (h - 1), rng.uniform(0.2, 0.8) * (w - 1)
        a = rng.uniform(0.15, 0.45) * max(h, w)
        b = rng.uniform(0.3, 0.9) * a
        th = rng.uniform(0, np.pi)
        u = (ii - ci) * np.cos(th) + (jj - cj) * np.sin(th)
        v = -(ii - ci) * np.sin(th) + (jj - cj) * np.cos(th)
        m = ((u / a) ** 2 + (v / max(b, 0.5)) ** 2 <= 1.0).astype(np.uint8)
        if f % 4 == 3:
            m[rng.random((h, w)) < 0.03] ^= 1
        if f % 7 == 6:
            m[rng.random((h, w)) < 0.02] = 2
        out[f] = m
    return out


def hand_frames():
    """[(name, (12, 14) uint8 frame, label)]: frames with a diagonal covariance or a trivial answer, compared in
    full. Blocks sit where their mean coordinates are exact in binary, as numpy's covariance needs for an exact 0."""
    h, w = 12, 14
    z = lambda: np.zeros((h, w), np.uint8)
    out = [("empty", z(), 1)]
    m = z(); m[5, 6] = 1; out.append(("one pixel", m, 1))
    m = z(); m[4, 6:8] = 1; out.append(("two in a row", m, 1))
    m = z(); m[4:6, 6] = 1; out.append(("two in a column", m, 1))
    m = z(); m[3:7, 4:8] = 1; out.append(("4x4 square", m, 1))
    m = z(); m[4:6, 3:9] = 1; out.append(("2x6", m, 1))
    m = z(); m[3:9, 4:6] = 1; out.append(("6x2", m, 1))
    m = z(); m[:, :] = 1; m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 0; out.append(("touching all four edges", m, 1))
    m = z(); m[:, 5:9] = 1; out.append(("band from the top edge to the bottom edge", m, 1))
    out.append(("full", np.ones((h, w), np.uint8), 1))
    m = np.tile(np.array([0, 1, 2, 5], np.uint8), (h, w))[:h, :w].copy(); m[2:6, 4:12] = 3
    out.append(("label 3 among others", m, 3))
    return out


def checkerboard(h, w):
    return ((np.add.outer(np.arange(h), np.arange(w)) & 1) == 0).astype(np.uint8)


def half_plane(h, w):
    m = np.zeros((h, w), np.uint8)
    m[: h // 2] = 1
    return m
