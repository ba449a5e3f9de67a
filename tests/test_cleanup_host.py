"""The mask cleanup rule on the host: the two restatements of tests/cleanup_oracle.py against each other, the
rule's known answers, and the argument checks that need no GPU."""
import os
import re

import numpy as np
import pytest

from tests import cleanup_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_restatements_agree_on_the_seeded_set():
    from scipy import ndimage as ndi
    several = filled = 0
    for frame, holesize in O.seeded_frames():
        a, b = O.clean_scipy(frame, holesize), O.clean_flood(frame, holesize)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], (frame.tolist(), holesize)
        several += ndi.label(frame == 1, structure=np.ones((3, 3)))[1] > 1
        filled += a[2] > 0
    assert several > 200 and filled > 200   # the set reaches the rule's branches


def test_cleaning_is_idempotent():
    for frame, holesize in O.seeded_frames(200, seed=1):
        once = O.clean_scipy(frame, holesize)[0]
        assert np.array_equal(O.clean_scipy(once, holesize)[0], once)
        assert np.array_equal(O.clean_flood(once, holesize)[0], once)


def test_filled_area_decides_between_a_ring_and_a_larger_blob():
    f = np.zeros((9, 20), np.uint8)
    f[1:8, 1:8] = 1
    f[2:7, 2:7] = 0        # ring: area 24, filled 49
    f[1:7, 10:16] = 1      # blob: area 36
    for fn in (O.clean_scipy, O.clean_flood):
        out, area, filled = fn(f, 4)
        assert area == 49 and filled == 0 and out.sum() == 24 and not out[:, 9:].any()
        out, area, filled = fn(f, 128)
        assert area == 49 and filled == 25 and out.sum() == 49


def test_small_frames_fill_completely_at_the_default():
    f = np.zeros((5, 7), np.uint8)
    f[2, 3] = 1
    assert O.clean_scipy(f)[0].all() and O.clean_flood(f)[0].all()


def test_spiral_helper_is_one_thin_component():
    from scipy import ndimage as ndi
    f = O.spiral(23, 31)
    assert ndi.label(f, structure=np.ones((3, 3)))[1] == 1 and ndi.label(f == 0)[1] == 1
    assert not (f[:-1, :-1] & f[1:, :-1] & f[:-1, 1:] & f[1:, 1:]).any()   # no 2 x 2 block: one pixel wide


@pytest.mark.parametrize("bad", [0, -1, 32768, 1.5, "3", None, True])
def test_holesize_is_checked_on_the_host(bad):
    from clasfv_amd import _lib
    with pytest.raises(ValueError, match="holesize"):
        _lib.clean_bits(bad)


def test_holesize_bits():
    from clasfv_amd import _lib
    assert _lib.clean_bits(1) == 0x200 | (1 << 16) and _lib.clean_bits(32767) == 0x200 | (32767 << 16)
    assert _lib.clean_bits(np.int64(128)) == 0x200 | (128 << 16) and _lib.clean_bits(32767) < 2 ** 31
    with pytest.raises(ValueError, match="labels"):
        _lib.check_clean_frame(209, 256, "labels")
    _lib.check_clean_frame(208, 256, "labels")
    _lib.check_clean_frame(224, 224, "labels")


def test_header_macros_equal_the_binding_constants():
    from clasfv_amd import _lib
    src = open(os.path.join(REPO, "include", "clasfv.h")).read()

    def macro(name):
        return re.search(r"#define\s+%s\b\s*(?:\([^)]*\))?\s+(.+)" % name, src).group(1).strip()
    assert int(macro("CLASFV_FUSE_CLEAN"), 0) == _lib.FUSE_CLEAN == 0x200
    assert int(macro("CLASFV_CLEAN_MAX_PIXELS"), 0) == _lib.CLEAN_MAX_PIXELS >= 224 * 224
    assert int(macro("CLASFV_CLEAN_DEFAULT_HOLES"), 0) == _lib.CLEAN_DEFAULT_HOLES == 128
    assert macro("CLASFV_FUSE_CLEAN_HOLES") == "((n) << 16)" and _lib.fuse_clean_holes(5) == 5 << 16
    assert _lib.FUSE_CLEAN & _lib.FUSE_FORCE_GENERIC == 0 and _lib.CLEAN_MAX_HOLES == (1 << 15) - 1
    # the kernel's LDS layout is what bounds the limit: 3 B per pixel beside its state, in 160 KiB
    hip = open(os.path.join(REPO, "fully-automated-multi-heartbeat-echocardiography-video-segmentation-and-motion-"
                            "tracking_amd", "csrc", "cleanup.hip")).read()
    state = int(re.search(r"CL_STATE_BYTES = (\d+)", hip).group(1))
    assert state + 3 * _lib.CLEAN_MAX_PIXELS <= 160 * 1024 and _lib.CLEAN_MAX_PIXELS < 0xFFFF


def test_cli_flags():
    import motion_segment as M
    a = M.parse_args(["-p", "x.npy"])
    assert a.cleanup is False and a.holesize == 128
    a = M.parse_args(["-p", "x.npy", "--cleanup", "--holesize", "5"])
    assert a.cleanup is True and a.holesize == 5
    for bad in ("0", "32768", "-3", "x"):
        with pytest.raises(SystemExit):
            M.parse_args(["-p", "x.npy", "--cleanup", "--holesize", bad])


def test_surface_refuses_bad_cleanup_arguments_before_any_device_work():
    """A bad holesize is a ValueError from every entry point that takes one, raised from host arithmetic (these
    run without a GPU: the video below never leaves the host)."""
    from clasfv_amd import dist, fuse_utils as FU
    video = np.zeros((3, 40, 16, 16), np.float32)

    def model(x):
        raise AssertionError("the model must not run")
    with pytest.raises(ValueError, match="holesize"):
        FU.segment_a_video_with_fusion(video, model, cleanup=True, holesize=0)
    with pytest.raises(ValueError, match="holesize"):
        dist.segment_videos_sharded([None], model, lengths=[40], cleanup=True, holesize=40000)
