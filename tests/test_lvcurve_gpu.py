"""clasfv_lv_geometry (csrc/lvgeom.hip) and its surface (echo.lv_curve, echo.ef_from_curve,
VideoStream.run(curves=True), the CLI's ``-c volume_curve``) against the host functions of echo.py.

The oracle, the robustness predicate that decides on which frames radii can be compared at all, the tolerance
and the seeded masks are in tests/lvcurve_oracle.py. The kernel is called through the ctypes ABI with its two
outputs between guard bands of all-ones bits (-1 is no pixel count, and the kernel's own NaN is the canonical
quiet one): after a launch the guards are intact and every output element is written.
"""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lvcurve_oracle as O
from tests.conftest import REPO, golden, unpack_labels

pytestmark = pytest.mark.gpu

GUARD = 1024
STRIDE = O.NP + 2
EHIP = -4  # CLASFV_EHIP: the only return code after which the device may have faulted
_ORACLE = {}


def dev():
    return torch.device("cuda", 0)


def lib():
    from clasfv_amd import _lib
    return _lib.load()


def oracle(key, make):
    """Oracle frames of a set, computed once per session."""
    if key not in _ORACLE:
        _ORACLE[key] = make()
    return _ORACLE[key]


def run_lv(frames, label=1, spacing=(1.0, 1.0), stream=None, offset=0):
    """One guarded clasfv_lv_geometry call on (F,H,W) uint8 frames -> (area (F,), geom (F,12)) numpy. ``offset``
    bytes move masks_dev off its allocation's alignment. A HIP error ends the session: nothing more is launched
    on a device that has faulted; a refusal of the arguments, which never touches the device, fails the test."""
    from clasfv_amd import _lib
    frames = np.ascontiguousarray(frames, np.uint8)
    f, h, w = frames.shape
    buf = torch.zeros(frames.size + offset + 64, dtype=torch.uint8, device=dev())
    masks = buf[offset:offset + frames.size]
    masks.copy_(torch.from_numpy(frames.reshape(-1)))
    area = torch.full((f + 2 * GUARD,), -1, dtype=torch.int32, device=dev())
    geom = torch.full((f * STRIDE + 2 * GUARD,), -1, dtype=torch.int64, device=dev())
    torch.cuda.synchronize()
    rc = lib().clasfv_lv_geometry(ctypes.c_void_p(masks.data_ptr()), f, h, w, label, spacing[0], spacing[1],
                                  ctypes.c_void_p(area.data_ptr() + 4 * GUARD), ctypes.c_void_p(geom.data_ptr() + 8 * GUARD),
                                  _lib.stream_ptr(stream, dev()))
    if rc == EHIP:
        pytest.exit(f"clasfv_lv_geometry: HIP error ({rc}) {lib().clasfv_last_error()}, stopping the session", returncode=3)
    assert rc == 0, f"clasfv_lv_geometry refused the call ({rc}): {lib().clasfv_last_error()}"
    try:
        torch.cuda.synchronize()
    except RuntimeError as ex:
        pytest.exit(f"clasfv_lv_geometry: HIP error, stopping the session: {ex}", returncode=3)
    a, g = area.cpu().numpy(), geom.cpu().numpy()
    for name, arr, n in (("area", a, f), ("geom", g, f * STRIDE)):
        assert (arr[:GUARD] == -1).all() and (arr[GUARD + n:] == -1).all(), f"write outside {name}"
        assert (arr[GUARD:GUARD + n] != -1).all(), f"{name}: elements left unwritten"
    return a[GUARD:GUARD + f].copy(), g[GUARD:GUARD + f * STRIDE].view(np.float64).reshape(f, STRIDE).copy()


def check(frames_oracle, area, geom, what, **kw):
    O.compare(frames_oracle, area, geom[:, 0], geom[:, 1:-1], geom[:, -1], what, **kw)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("h,w", O.SIZES, ids=lambda v: str(v))
def test_generated_masks_vs_host_functions(h, w):
    """~100 seeded tilted ellipses per frame size (noisy ones with several components, empty slabs and NaN
    radii; some with pixels of value 2, which are background), all in ONE launch, against get2dPucks and
    _disk_volume per frame. The same frames in reversed order and alone (F = 1) give the same bits."""
    masks = O.ellipse_masks(h, w)
    area, geom = run_lv(masks)
    check(oracle(("ellipses", h, w), lambda: O.oracle_frames(masks)), area, geom, f"{h}x{w}")
    ra, rg = run_lv(masks[::-1])
    assert np.array_equal(ra[::-1], area) and same_bits(rg[::-1], geom), "results depend on the place in the batch"
    for i in range(len(masks)):
        a1, g1 = run_lv(masks[i:i + 1])
        assert a1[0] == area[i] and same_bits(g1[0], geom[i]), f"frame {i} alone differs from the batch"


def test_hand_made_frames_in_full():
    """Frames with a diagonal covariance or a trivial answer, robust by construction, compared in full: empty,
    one pixel, two pixels in a row and in a column, a square (equal variances: the j axis comes first), 2x6 and
    6x2 rectangles, a shape touching all four frame edges, a full frame (NaN) and label 3 among other values."""
    hand = O.hand_frames()
    for label in sorted({lab for _, _, lab in hand}):
        names = [n for n, _, lab in hand if lab == label]
        frames = np.stack([fr for _, fr, lab in hand if lab == label])
        orc = O.oracle_frames(frames, label)
        assert all(f.robust for f in orc)
        area, geom = run_lv(frames, label)
        check(orc, area, geom, f"label {label}: {names}")
    by_name = {n: fr for n, fr, _ in hand}
    area, geom = run_lv(np.stack([by_name["empty"], by_name["one pixel"], by_name["full"]]))
    assert area.tolist() == [0, 1, 12 * 14]
    assert geom[0].tolist() == [1.0] + [0.0] * 11 and geom[1].tolist() == [0.0] * 12 and np.isnan(geom[2]).all()


@pytest.mark.parametrize("h,w", [(112, 112), (200, 200), (403, 404)], ids=lambda v: str(v))
def test_every_rim_count_is_served(h, w):
    """The frames at which a rim-list capacity or an LDS size can be wrong: a checkerboard and row stripes
    (every pixel a rim pixel) and a half-plane, at the product size (every rim fits the kernel's rim list), at
    200 x 200 (the all-rim frames exceed the list and are scanned from their flag bytes, the half-plane beside
    them in the same launch is listed) and just under CLASFV_LV_MAX_PIXELS (no room for a list at all). Area
    and length against the host functions on all of them, radii and volume where robust: the half-plane and the
    stripes are (diagonal covariance), the checkerboard ties with its cuts by construction and is the one frame
    the 10 % cap does not count."""
    from clasfv_amd.echo import thick_boundary
    stripes = np.zeros((h, w), np.uint8)
    stripes[::2] = 1
    frames = np.stack([O.checkerboard(h, w), O.half_plane(h, w), stripes])
    orc = oracle(("rim", h, w), lambda: O.oracle_frames(frames))
    assert orc[1].robust and orc[2].robust
    assert all(thick_boundary(frames[k]).all() for k in (0, 2))  # every pixel is a rim pixel
    area, geom = run_lv(frames)
    check(orc, area, geom, f"rim {h}x{w}", rim_count=True)
    assert np.isfinite(geom[1:]).all()


def test_more_frames_than_workgroups():
    """F above the 65536 workgroups of a launch: a workgroup then serves several frames in turn, re-zeroing its
    state and restaging the frame, also after a frame that ended early (empty, one pixel, full). 66,000 frames
    of 4 x 4 in one launch give the bits of the same frames in four smaller launches; a sample against the host
    functions (area everywhere, the rest where robust: tiny frames tie often, so no cap here -- the comparison
    that counts is the bit identity)."""
    rng = np.random.default_rng(11)
    f = 66000
    masks = (rng.random((f, 4, 4)) < rng.random((f, 1, 1))).astype(np.uint8)
    masks[::5] = 0
    masks[1::5] = 0
    masks[1::5, 2, 1] = 1
    masks[2::5] = 1
    area, geom = run_lv(masks)
    assert np.array_equal(area, masks.reshape(f, -1).sum(1))
    step = f // 4
    for s in range(0, f, step):
        a, g = run_lv(masks[s:s + step])
        assert np.array_equal(a, area[s:s + step]) and same_bits(g, geom[s:s + step]), f"frames {s}.."
    for i in list(range(20)) + list(range(65530, 65560)) + list(range(f - 20, f)):
        o = O.oracle_frame(masks[i] == 1)
        assert area[i] == o.area
        if o.robust:
            np.testing.assert_allclose(geom[i], [o.length, *o.radii, o.volume], rtol=O.RTOL, atol=0, equal_nan=True,
                                       err_msg=f"frame {i}")


def test_permuted_and_strided_masks():
    """lv_curve hands the library a dense (F,H,W) block whatever the layout of its input: permuted views (a
    (T,N,H,W) stack seen batch-first, H and W transposed), strided and cropped views, of int64, int32 and uint8
    masks, give the bits of their .contiguous() copies and the areas torch counts."""
    from clasfv_amd import echo
    base = torch.from_numpy(O.ellipse_masks(13, 29, count=24, seed=9)).to(dev()).view(4, 6, 13, 29)
    for dtype in (torch.int64, torch.int32, torch.uint8):
        b = base.to(dtype)
        for k, v in enumerate((b.transpose(0, 1), b.transpose(2, 3), b[:, ::2], b[..., 1:-2, 3:20])):
            assert not v.is_contiguous()
            got, ref = echo.lv_curve(v).cpu(), echo.lv_curve(v.contiguous()).cpu()
            assert got.area.shape == tuple(v.shape[:-2]) and bool(ref.area.any())
            assert np.array_equal(got.area, ref.area) and same_bits(got.geom, ref.geom), (dtype, k)
            assert np.array_equal(got.area, (v == 1).sum(dim=(-2, -1)).cpu().numpy()), (dtype, k)


def test_spacing():
    masks = O.ellipse_masks(13, 29)
    area, geom = run_lv(masks, spacing=(0.5, 2.0))
    check(oracle(("spacing",), lambda: O.oracle_frames(masks, spacing=(0.5, 2.0))), area, geom, "spacing (0.5, 2.0)")


def test_misaligned_masks_and_non_default_stream():
    masks = O.ellipse_masks(31, 17)
    area, geom = run_lv(masks)
    a1, g1 = run_lv(masks, offset=1)
    assert np.array_equal(a1, area) and same_bits(g1, geom)
    s = torch.cuda.Stream(dev())
    a2, g2 = run_lv(masks, stream=s, offset=3)
    assert np.array_equal(a2, area) and same_bits(g2, geom)


@pytest.mark.parametrize("name", ["northstar_c1", "northstar_c1_random", "northstar_c1_deep"])
def test_northstar_curve_and_ef(name):
    """The config[1] fused masks (200 x 112 x 112) through echo.lv_curve: the curve against the host functions,
    and ef_from_curve on the device curve gives the fixture's ED / ES pairs exactly and its EFs within 1e-6 EF
    points (what 1e-9 on length and radii allows through the quotient, with a factor of a few in hand)."""
    from clasfv_amd import echo
    g = golden(name + ".npz")
    masks = unpack_labels(g, "fused_simple")
    curve = echo.lv_curve(torch.from_numpy(masks.astype(np.uint8)).to(dev()))
    assert curve.area.dtype == torch.int32 and curve.volume.dtype == torch.float64 and curve.radii.shape == (200, 10)
    c = curve.cpu()
    O.compare(oracle((name,), lambda: O.oracle_frames(masks)), c.area, c.length, c.radii, c.volume, name)
    efs, pairs = echo.ef_from_curve(curve.area, curve.volume, name, return_edes=True)
    assert np.array(pairs, np.int64).reshape(-1, 2).tolist() == g["pairs_simple"].reshape(-1, 2).tolist()
    ref = np.asarray(g["ef_simple"], np.float64)
    assert len(efs) == len(ref)
    print(name, "max |EF - fixture| =", np.abs(np.array(efs) - ref).max() if len(ref) else 0.0)
    np.testing.assert_allclose(np.array(efs, np.float64), ref, rtol=0, atol=1e-6)
    # (N,T,H,W) int64 masks: compared with the label on the device first, the same curve in the masks' shape
    wide = echo.lv_curve(torch.from_numpy(masks).to(dev()).view(2, 100, 112, 112))
    assert wide.area.shape == (2, 100) and wide.radii.shape == (2, 100, 10)
    assert torch.equal(wide.area.view(-1), curve.area) and same_bits(wide.cpu().geom.reshape(200, 12), c.geom)


@pytest.fixture(scope="module")
def echo_model():
    from clasfv_amd.model import R2plus1D_18_MotionNet
    return R2plus1D_18_MotionNet(pretrained=False, weights="echo")


def test_video_stream_curves(echo_model):
    """VideoStream.run(curves=True): masks bit-identical to curves=False, curves bit-identical to lv_curve on
    the returned masks -- on the host path (one pinned transfer) and with return_device=True."""
    import clasfv_amd.synthetic as S
    from clasfv_amd import echo
    from clasfv_amd.stream import VideoStream
    vids = [S.echo_video_uint8(T, seed=80 + T) for T in (40, 48)]
    vs = VideoStream(echo_model, num_clips=2, fuse_method="simple")
    plain = vs.run(vids)
    got = vs.run(vids, curves=True)
    on_dev = vs.run(vids, curves=True, return_device=True)
    assert len(got) == len(on_dev) == 2
    for p, (m, c), (dm, dc) in zip(plain, got, on_dev):
        assert m.dtype == np.int64 and np.array_equal(m, p) and np.array_equal(dm.cpu().numpy(), p)
        assert m.any(), "the synthetic video has an LV"
        ref = echo.lv_curve(torch.from_numpy(m).to(dev())).cpu()
        assert dc.area.is_cuda and dc.volume.is_cuda
        for cur in (c, dc.cpu()):
            assert cur.area.dtype == np.int32 and np.array_equal(cur.area, ref.area) and same_bits(cur.geom, ref.geom)
            assert cur.radii.shape == (len(p), 10) and cur.volume.shape == (len(p),)


def test_curve_of_a_tracked_video():
    """lv_curve(warp.track_labels(...)), an int64 video, equals lv_curve of the same video cast to uint8."""
    from clasfv_amd import echo, warp
    rng = np.random.default_rng(5)
    n, t, h, w = 2, 6, 24, 32
    labels = torch.zeros((n, t, h, w), dtype=torch.int64, device=dev())
    seed = O.ellipse_masks(h, w, count=n, seed=3).astype(np.int64)
    labels[:, 2] = torch.from_numpy(seed).to(dev())
    motion = torch.from_numpy((rng.standard_normal((n, 4, t, h, w)) * 0.04).astype(np.float32)).to(dev())
    tracked = warp.track_labels(labels, motion, 2)
    assert tracked.dtype == torch.int64 and bool((tracked == 1).any())
    a, b = echo.lv_curve(tracked).cpu(), echo.lv_curve(tracked.to(torch.uint8)).cpu()
    assert a.area.shape == (n, t) and np.array_equal(a.area, b.area) and same_bits(a.geom, b.geom)
    assert np.array_equal(a.area, (tracked == 1).sum(dim=(2, 3)).cpu().numpy())


@pytest.mark.timeout(400)
def test_cli_volume_curve(tmp_path):
    """``-c volume_curve`` writes <name>_lv_volume_curve.pkl, a dict of numpy arrays equal to lv_curve on the
    masks of ``-c binary_video``; the ``-c binary`` pickles are byte-identical with and without the keyword."""
    import clasfv_amd.synthetic as S
    from clasfv_amd import echo
    vid = tmp_path / "clip32.npy"
    np.save(vid, S.echo_video_uint8(32, seed=7))
    outs = {}
    for key, content in (("with", "binary,binary_video,volume_curve"), ("without", "binary")):
        outs[key] = tmp_path / key
        outs[key].mkdir()
        r = subprocess.run([sys.executable, "motion_segment.py", "-p", str(vid), "--synthetic-weights", "1234", "-f", "1",
                            "--no-strict-reference", "-c", content, "-o", str(outs[key])],
                           capture_output=True, text=True, timeout=180, cwd=REPO)
        assert r.returncode == 0, r.stderr[-3000:]
    binary = sorted(f for f in os.listdir(outs["without"]))
    assert sorted(os.listdir(outs["with"])) == sorted(binary + ["clip32_whole_video_segmentation.pkl",
                                                                "clip32_lv_volume_curve.pkl"])
    for f in binary:
        assert (outs["with"] / f).read_bytes() == (outs["without"] / f).read_bytes(), f
    masks = pickle.load(open(outs["with"] / "clip32_whole_video_segmentation.pkl", "rb"))
    curve = pickle.load(open(outs["with"] / "clip32_lv_volume_curve.pkl", "rb"))
    ref = echo.lv_curve(torch.from_numpy(masks).to(dev())).asdict()
    assert sorted(curve) == ["area", "length", "radii", "volume"] and masks.shape == (32, 112, 112)
    for k, v in curve.items():
        assert isinstance(v, np.ndarray) and v.dtype == ref[k].dtype and v.shape == ref[k].shape, k
        assert np.array_equal(v, ref[k], equal_nan=True), k
    assert curve["area"].dtype == np.int32 and curve["radii"].shape == (32, 10) and curve["area"].any()
