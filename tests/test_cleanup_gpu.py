"""CLASFV_FUSE_CLEAN (csrc/cleanup.hip) through the C ABI, between guard bands, byte for byte against the host
restatements of tests/cleanup_oracle.py; and the Python surface that carries the flag.

Every frame goes through clasfv_fuse_votes with K = 1 and CLASFV_FUSE_MAJORITY, which hands a single pass's bytes
on unchanged (2s included), so the bytes compared are the cleanup kernel's alone. Small frames take small hole
thresholds: a frame under 128 pixels with any member fills completely at the default, which one case asserts.
"""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import abi_audit as A
from tests import cleanup_oracle as O
from tests import stream_order as SO
from tests.golden.fake_model import fake_model
from tests.test_plumbing_gpu import EBADSHAPE, EINVAL, Guarded, _refused, dev, launch, ptr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEANUP_HIP = os.path.join(REPO, "fully-automated-multi-heartbeat-echocardiography-video-segmentation-and-motion-"
                           "tracking_amd", "csrc", "cleanup.hip")
CLEAN, GENERIC = 0x200, 0x100
MAX_PIXELS = 53248
METHODS = {"majority": 0, "itkvoting": 3, "simple": 1, "simple-generic": 1 | GENERIC, "staple": 2}


def holes(n):
    return n << 16


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def clean_gpu(frames, holesize=None):
    """(F,H,W) uint8 frames through one flagged K = 1 majority call; ``holesize`` None leaves the bits 0."""
    frames = np.asarray(frames, np.uint8)
    f, h, w = frames.shape
    lab, out = D(frames), Guarded(f * h * w, torch.uint8)
    method = CLEAN | (holes(holesize) if holesize is not None else 0)
    assert launch("clasfv_fuse_votes", ptr(lab), 1, f, 1, h, w, method, ptr(out.t)) == 0
    assert out.guards_intact() and torch.equal(lab, D(frames))
    return out.t.view(f, h, w).cpu().numpy()


def check(frame, holesize, flood=True):
    frame = np.asarray(frame, np.uint8)
    want = O.clean_scipy(frame, holesize)[0]
    if flood:
        assert np.array_equal(want, O.clean_flood(frame, holesize)[0])
    got = clean_gpu(frame[None], holesize)[0]
    assert np.array_equal(got, want), f"{frame.shape} holesize {holesize}: {int((got != want).sum())} pixels differ"
    return got


def Z(h, w):
    return np.zeros((h, w), np.uint8)


# ---- known answers ----------------------------------------------------------------------------------------
def test_degenerate_shapes():
    assert check([[1]], 128).tolist() == [[1]] and check([[0]], 128).tolist() == [[0]]
    assert check([[2]], 1).tolist() == [[2]]
    line = np.array([[1, 0, 1, 1, 0, 0, 1, 1, 1]], np.uint8)
    for f in (line, line.T.copy()):
        assert check(f, 1).ravel().tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1]   # the largest run; nothing filled
        assert check(f, 2).ravel().tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1]   # the six others are one component
        assert check(f, 7).ravel().tolist() == [1] * 9
    assert check(np.ones((5, 7), np.uint8), 3).all()
    assert not check(Z(5, 7), 128).any()                                     # no member: unchanged
    assert (check(np.full((5, 7), 2, np.uint8), 128) == 2).all()             # only 2s: unchanged


def test_a_small_frame_fills_completely_at_the_default():
    f = Z(5, 7)
    f[1, 2] = f[3, 5] = 1
    f[0, 0] = 2
    want = O.clean_scipy(f, 128)[0]
    assert want.all() and np.array_equal(clean_gpu(f[None])[0], want)        # no threshold bits: 128


def ring_and_blob():
    f = Z(9, 20)
    f[1:8, 1:8] = 1
    f[2:7, 2:7] = 0
    f[1:7, 10:16] = 1
    return f


def test_filled_area_decides():
    f = ring_and_blob()
    out = check(f, 4)
    assert out.sum() == 24 and not out[:, 9:].any() and not out[2:7, 2:7].any()   # the ring is kept, its hole stays
    assert check(f, 128).sum() == 49 and check(f, 26)[1:8, 1:8].all()
    assert check(f, 25).sum() == 24                                                 # a hole of holesize pixels stays


def test_nested_rings():
    f = Z(20, 34)
    f[1:16, 1:16] = 1
    f[2:15, 2:15] = 0         # outer ring: area 56, filled 225 with the inner ring inside it
    f[5:12, 5:12] = 1
    f[6:11, 6:11] = 0         # inner ring: area 24, filled 49
    f[2:12, 20:30] = 1        # blob: area 100, the largest plain area; both rings can still beat it
    out = check(f, 2)
    assert out.sum() == 56 and out[1, 1] == 1 and out[5, 5] == 0
    g = f.copy()
    g[1:16, 1:16] = 0
    g[5:12, 5:12] = f[5:12, 5:12]
    assert check(g, 2).sum() == 100          # without the outer ring the blob wins: 100 > 49


def test_the_two_connectivities():
    d = Z(12, 24)
    for i in range(7):
        for j in range(7):
            if abs(i - 3) + abs(j - 3) == 3:
                d[2 + i, 2 + j] = 1          # a diamond ring of 12 pixels that touch at corners only
    alone = check(d, 14)
    assert alone.sum() == 25                 # one component; its 13 interior pixels are closed under 4-connectivity
    assert check(d, 13).sum() == 12
    d[3:7, 14:18] = 1                        # a solid blob of 16: more than 12, less than 12 + 13
    out = check(d, 2)
    assert out.sum() == 16 and not out[:, :12].any()   # the interior leaks through the diagonal gaps: filled area 12


def test_corner_pocket():
    f = Z(8, 8)
    f[3, 0:4] = 1
    f[0:4, 3] = 1                            # a wall that cuts a 3 x 3 pocket off the corner
    assert check(f, 10)[0:3, 0:3].all() and check(f, 10).sum() == 7 + 9
    assert not check(f, 9)[0:3, 0:3].any()


def _ring_with_hole(n):
    f = Z(16, 24)
    f[2:12, 2:20] = 1
    f[3:11, 3:19] = 0                        # 128 pixels inside
    inner = np.zeros(128, np.uint8)
    inner[:128 - n] = 1                         # whole rows from the top, then part of one: the hole stays one piece
    f[3:11, 3:19] = inner.reshape(8, 16)
    assert (f[3:11, 3:19] == 0).sum() == n
    return f


@pytest.mark.parametrize("holesize", [1, 2, 128])
def test_threshold(holesize):
    if holesize > 1:
        f = _ring_with_hole(holesize - 1)
        assert check(f, holesize)[2:12, 2:20].all()
    f = _ring_with_hole(holesize)
    out = check(f, holesize)
    assert (out[3:11, 3:19] == 0).sum() == holesize and np.array_equal(out, f)


def test_tie_goes_to_the_first_in_row_major_order():
    f = Z(9, 12)
    f[4:7, 1:4] = 1
    f[2:5, 7:10] = 1                         # the right blob starts in row 2: it comes first
    out = check(f, 1)
    assert out.sum() == 9 and out[2:5, 7:10].all()
    out = check(f[::-1].copy(), 1)
    assert out.sum() == 9 and out[2:5, 1:4].all()


def test_twos_pass_through_and_are_filled_over():
    f = Z(14, 14)
    f[2:9, 2:9] = 1
    f[4:7, 4:7] = 0
    f[5, 5] = 2
    f[12, 1] = f[0, 13] = 2
    f[11, 11] = 1
    out = check(f, 10)
    assert out[5, 5] == 1 and out[12, 1] == 2 and out[0, 13] == 2 and out[11, 11] == 0
    assert check(f, 9)[5, 5] == 2


@pytest.mark.parametrize("side", [112, 224])
def test_worst_case_spiral(side):
    """A one-pixel-wide spiral: the longest way round for any propagation that goes a hop at a time. The kernel
    labels by union-find, so the frame costs one pass like any other."""
    f = O.spiral(side, side)
    assert np.array_equal(check(f, 128, flood=False), f)
    g = 1 - f                                # the corridor between its arms, as the member
    check(g, 128, flood=False)


# ---- sizes -------------------------------------------------------------------------------------------------
def _blobs(h, w, seed, density):
    r = np.random.default_rng(seed)
    f = (r.random((h, w)) < density).astype(np.uint8)
    f[(r.random((h, w)) < 0.02) & (f == 0)] = 2
    yy, xx = np.mgrid[0:h, 0:w]
    core = ((yy - h / 2) / (h / 4 + 1)) ** 2 + ((xx - w / 2) / (w / 5 + 1)) ** 2 <= 1
    f[core & (r.random((h, w)) < 0.9)] = 1
    return f


SIZES = [(5, 7), (33, 65), (112, 112), (224, 224), (208, 256)]
assert SIZES[-1][0] * SIZES[-1][1] == MAX_PIXELS


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes(hw):
    h, w = hw
    small = h * w < 1000
    for seed, density, holesize in ((1, 0.1, 3), (2, 0.3, 5), (3, 0.55, 128)):
        check(_blobs(h, w, seed, density), min(holesize, 2) if h * w < 128 else holesize, flood=small)
    if not small:
        r = np.random.default_rng(9)         # noise below the percolation threshold: many candidates, many floods
        check((r.random((h, w)) < 0.33).astype(np.uint8), 4, flood=False)


def test_one_past_the_limit_is_refused():
    h, w = 209, 256
    lab = torch.ones((2, h, w), dtype=torch.uint8, device=dev())
    for method in (CLEAN, CLEAN | holes(5), 1 | CLEAN, 2 | CLEAN | GENERIC):
        _refused("clasfv_fuse_votes", (ptr(lab), 1, 2, 1, h, w, method), Guarded(2 * h * w, torch.uint8), EBADSHAPE)
    out = Guarded(2 * h * w, torch.uint8)    # the same call without the flag is served
    assert launch("clasfv_fuse_votes", ptr(lab), 1, 2, 1, h, w, 0, ptr(out.t)) == 0 and bool(out.t.all())


def test_refusals():
    lab = torch.ones((2, 6, 5, 7), dtype=torch.uint8, device=dev())
    bit31 = -(1 << 31)
    for method in (holes(5), holes(5) | 1, holes(32767) | GENERIC | 1, bit31, bit31 | CLEAN, bit31 | CLEAN | holes(5),
                   0x400, 0x400 | CLEAN, 0x8000 | CLEAN, 4 | CLEAN, 0x80 | CLEAN | holes(5)):
        _refused("clasfv_fuse_votes", (ptr(lab), 2, 6, 1, 5, 7, method), Guarded(6 * 35, torch.uint8), EINVAL)


# ---- the batch ---------------------------------------------------------------------------------------------
def test_batch_independence():
    """A frame's bytes do not depend on F or on its place: reversed, alone, and in a launch longer than the grid."""
    frames = np.stack([np.pad(f, ((0, 23 - f.shape[0]), (0, 23 - f.shape[1]))) for f, _ in O.seeded_frames(60, seed=5)])
    frames[7] = 0
    want = O.clean_video(frames, 5)
    got = clean_gpu(frames, 5)
    assert np.array_equal(got, want)
    assert np.array_equal(clean_gpu(frames[::-1].copy(), 5)[::-1], got)
    assert np.array_equal(clean_gpu(got, 5), got)                    # idempotent
    for i in (0, 7, 31, 59):
        assert np.array_equal(clean_gpu(frames[i:i + 1], 5)[0], got[i])
    grid = int(re.search(r"CL_GRID_MAX = (\d+)", open(CLEANUP_HIP).read()).group(1))
    n = grid + 61                                                    # the grid loops: block b takes frames b, b + grid
    long = clean_gpu(np.concatenate([frames] * (n // 60 + 1))[:n], 5)
    assert np.array_equal(long, np.concatenate([got] * (n // 60 + 1))[:n])


def _votes(k, t, h, w, seed):
    """K noisy passes around an ellipse, with islands and holes that survive the vote."""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    truth = (((yy - h / 2) / (h / 3)) ** 2 + ((xx - w / 2) / (w / 4)) ** 2 <= 1).astype(np.uint8)
    truth = np.repeat(truth[None], t, 0)
    truth[:, 0, 0] = truth[:, h - 1, w - 2] = 1
    truth[:, h // 2, w // 2] = 0
    flip = r.random((k, t, h, w)) < 0.15
    return (truth[None] ^ flip).astype(np.uint8)


@pytest.mark.parametrize("k", [2, 17])
@pytest.mark.parametrize("name", sorted(METHODS))
def test_composition(name, k):
    """The flagged call is the unflagged call followed by a flagged K = 1 call, byte for byte (no oracle)."""
    t, h, w, method = 6, 12, 16, METHODS[name]
    lab = D(_votes(k, t, h, w, k))
    plain, both = Guarded(t * h * w, torch.uint8), Guarded(t * h * w, torch.uint8)
    assert launch("clasfv_fuse_votes", ptr(lab), k, t, 1, h, w, method, ptr(plain.t)) == 0
    assert launch("clasfv_fuse_votes", ptr(lab), k, t, 1, h, w, method | CLEAN | holes(3), ptr(both.t)) == 0
    assert plain.guards_intact() and both.guards_intact()
    fused = plain.t.view(t, h, w).cpu().numpy()
    want = clean_gpu(fused, 3)
    assert np.array_equal(both.t.view(t, h, w).cpu().numpy(), want)
    assert np.array_equal(want, O.clean_video(fused, 3)) and not np.array_equal(want, fused)


def test_flagged_call_behind_a_blocked_stream():
    from tests.test_stream_order_gpu import case_of, lib, pair
    k, t, h, w = 3, 12, 8, 12
    lab = pair(lambda r: (r.random((k, t, h, w)) < 0.5).astype(np.uint8), "fuse-clean")
    out = torch.empty((t, h, w), dtype=torch.uint8, device=dev())

    def call():
        SO.ok(lib().clasfv_fuse_votes(ptr(lab[0]), k, t, 1, h, w, 1 | CLEAN | holes(3), ptr(out), SO.current_ptr()),
              "clasfv_fuse_votes")
        return [out]
    SO.run_behind_blocker(case_of("clasfv_fuse_votes[simple+clean]", call, [lab], [out]))


# ---- the Python surface ------------------------------------------------------------------------------------
def speckled(t=24):
    """(ellipse video, the same with planted islands, none 8-adjacent to the ellipse and all smaller than it)."""
    import clasfv_amd.synthetic as S
    clean = S.ellipse_masks(t).astype(np.uint8)
    dirty = clean.copy()
    dirty[:, 3:6, 4:9] = 1
    dirty[::2, 100:104, 100:103] = 1
    dirty[:, 56, 2] = 1
    dirty[1::3, 108, 60:70] = 1
    assert not (clean[:, :12].any() or clean[:, 100:].any() or clean[:, :, :12].any() or clean[:, :, 100:].any())
    return clean, dirty


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def test_cleanup_restores_the_curve():
    from clasfv_amd import echo
    clean, dirty = speckled()
    for masks in (D(dirty), D(dirty.astype(np.int64)), D(dirty * 3)):
        label = 3 if int(masks.max()) == 3 else 1
        out = echo.cleanup_masks(masks, label=label)
        assert out.dtype == torch.uint8 and out.shape == masks.shape and np.array_equal(out.cpu().numpy(), clean)
    assert np.array_equal(echo.cleanup_masks(D(dirty[3])).cpu().numpy(), clean[3])     # (H,W)
    good, bad, fixed = (echo.lv_curve(D(m)).cpu() for m in (clean, dirty, echo.cleanup_masks(D(dirty)).cpu().numpy()))
    assert np.array_equal(fixed.area, good.area) and same_bits(fixed.geom, good.geom)
    assert not np.array_equal(bad.area, good.area)
    assert not np.allclose(bad.volume, good.volume, rtol=0.05, equal_nan=True)   # the defect the cleanup removes
    with pytest.raises(ValueError, match="holesize"):
        echo.cleanup_masks(D(dirty), holesize=0)
    with pytest.raises(ValueError, match="masks"):
        echo.cleanup_masks(torch.zeros((1, 209, 256), dtype=torch.uint8, device=dev()))
    with pytest.raises(ValueError, match="masks"):
        echo.cleanup_masks(torch.from_numpy(dirty))


def test_pointer_audit(monkeypatch):
    """The flagged calls stay inside clasfv_fuse_votes' footprint rule: reads K*T*H*W, writes T'*H*W."""
    from clasfv_amd import _lib, echo, fuse_utils as FU
    _, dirty = speckled(6)
    with monkeypatch.context() as mp:
        aud = A.install(mp, _lib)
        echo.cleanup_masks(D(dirty))
        echo.cleanup_masks(D(dirty[0].astype(np.int64)), holesize=7)
        votes = D(_votes(3, 8, 12, 16, 1))
        for method in ("majority", "simple", "staple", "itkvoting"):
            a = FU.fuse_votes(votes, 2, method, cleanup=True, holesize=3)
            b = FU.fuse_votes(FU.fuse_votes(votes, 2, method)[None], 1, "majority", cleanup=True, holesize=3)
            assert a.shape == (7, 12, 16) and torch.equal(a, b)
        FU.fuse_votes(votes.to(torch.int64)[:, :, ::2], 1, "simple", force_generic=True, cleanup=True)
        torch.cuda.synchronize()
        assert aud.calls["clasfv_fuse_votes"] == 2 + 4 * 3 + 1
    with pytest.raises(ValueError, match="labels"):
        FU.fuse_votes(torch.zeros((1, 1, 209, 256), dtype=torch.uint8, device=dev()), 1, "majority", cleanup=True)
    with pytest.raises(ValueError, match="holesize"):
        FU.fuse_votes(votes, 1, cleanup=True, holesize=32768)


def _videos(n=2, t=40):
    r = np.random.default_rng(11)
    return [r.integers(0, 256, (t, 20, 24, 3), dtype=np.uint8) for _ in range(n)]


def test_video_stream_cleans_before_the_curve():
    from clasfv_amd import echo
    from clasfv_amd.stream import VideoStream, segment_videos
    vids = _videos()
    kw = dict(num_clips=2, height=16, width=16, fuse_method="majority")
    plain = VideoStream(fake_model, **kw).run(vids)
    got = VideoStream(fake_model, cleanup=True, holesize=6, **kw).run(vids, curves=True)
    again = segment_videos(vids, fake_model, 2, 1, "majority", 16, 16, curves=True, cleanup=True, holesize=6)
    changed = 0
    for p, (m, c), (m2, c2) in zip(plain, got, again):
        want = echo.cleanup_masks(D(p), holesize=6)
        ref = echo.lv_curve(want).cpu()
        assert m.dtype == np.int64 and np.array_equal(m, want.cpu().numpy()) and np.array_equal(m, m2)
        assert np.array_equal(c.area, ref.area) and np.array_equal(c.geom, ref.geom, equal_nan=True)
        assert np.array_equal(c2.geom, ref.geom, equal_nan=True)
        changed += int((m != p).sum())
    assert changed > 0


@pytest.mark.parametrize("strict", [True, False])
def test_segment_a_video_with_fusion_cleans_every_frame(strict):
    from clasfv_amd import echo, fuse_utils as FU
    video = np.random.default_rng(12).uniform(0, 1, (3, 70, 16, 16)).astype(np.float32)
    kw = dict(step=2, num_clips=3, fuse_method="itkvoting", strict_reference=strict)
    plain = FU.segment_a_video_with_fusion(video, fake_model, **kw)
    got = FU.segment_a_video_with_fusion(video, fake_model, cleanup=True, holesize=4, **kw)
    assert got.dtype == np.int64 and got.shape == plain.shape and got.shape[0] == (69 if strict else 70)
    assert np.array_equal(got, O.clean_video(plain.astype(np.uint8), 4)) and not np.array_equal(got, plain)
    on_dev = FU.segment_a_video_with_fusion_device(video, fake_model, cleanup=True, holesize=4, **kw)
    assert on_dev.dtype == torch.uint8 and np.array_equal(on_dev.cpu().numpy(), got)


def test_segment_videos_sharded_cleans_on_the_owner():
    from clasfv_amd import dist as DI, echo
    r = np.random.default_rng(13)
    vids = [D(r.uniform(0, 1, (3, t, 16, 16)).astype(np.float32)) for t in (40, 70)]
    plain = DI.segment_videos_sharded(vids, fake_model, num_clips=2, fuse_method="simple")
    got = DI.segment_videos_sharded(vids, fake_model, num_clips=2, fuse_method="simple", cleanup=True, holesize=4)
    assert sorted(got) == [0, 1]
    for i in got:
        assert torch.equal(got[i], echo.cleanup_masks(plain[i], holesize=4)) and not torch.equal(got[i], plain[i])


def test_cli_cleanup(tmp_path):
    """``--cleanup --holesize N``: the pickles hold cleanup_masks of what the CLI writes without the flags."""
    import clasfv_amd.synthetic as S
    from clasfv_amd import echo
    vid = tmp_path / "clip32.npy"
    frames = S.echo_video_uint8(32, seed=7)
    frames[:, 4:8, 4:8] = 0          # dark patches away from the LV: islands for the synthetic weights' threshold
    np.save(vid, frames)
    outs = {}
    for key, extra in (("plain", []), ("clean", ["--cleanup", "--holesize", "40"])):
        outs[key] = tmp_path / key
        outs[key].mkdir()
        r = subprocess.run([sys.executable, "motion_segment.py", "-p", str(vid), "--synthetic-weights", "1234", "-f", "1",
                            "--no-strict-reference", "-c", "binary_video,volume_curve", "-o", str(outs[key])] + extra,
                           capture_output=True, text=True, timeout=180, cwd=REPO)
        assert r.returncode == 0, r.stderr[-3000:]
    plain, clean = (pickle.load(open(outs[k] / "clip32_whole_video_segmentation.pkl", "rb")) for k in ("plain", "clean"))
    want = echo.cleanup_masks(D(plain), holesize=40)
    assert clean.dtype == np.int64 and np.array_equal(clean, want.cpu().numpy())
    curve = pickle.load(open(outs["clean"] / "clip32_lv_volume_curve.pkl", "rb"))
    ref = echo.lv_curve(want).asdict()
    assert all(np.array_equal(curve[k], ref[k], equal_nan=True) for k in ref)
