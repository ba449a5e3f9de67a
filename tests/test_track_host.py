"""CPU tests of clasfv_track's argument checks (they precede any HIP call, so they need no GPU), of the
CLASFV_TRACK_* constants, and of the reference-run fixture tests/golden/track.npz."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import REPO, golden
from tests.golden.make_golden import REF

HEADER = os.path.join(REPO, "include", "clasfv.h")
EINVAL, EBADSHAPE = -1, -2


def test_track_refusals_need_no_gpu():
    """Null pointers, P < 1, t_step other than +-1, a used frame outside [0, T), an unknown mode, empty
    dimensions and out overlapping img are refused with CLASFV_EINVAL, planes or batches of 2^31 elements with
    CLASFV_EBADSHAPE, each with a message -- before any HIP call (the pointers here are never dereferenced)."""
    from clasfv_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    ok = dict(img=P(0x10000), n=2, c=2, h=5, w=9, mot=P(0x20000), sn=4 * 4 * 45, sc=4 * 45, st=45, t=4, t0=0, step=1,
              count=3, mode=_lib.TRACK_BILINEAR, out=P(0x40000), stream=None)
    order = ["img", "n", "c", "h", "w", "mot", "sn", "sc", "st", "t", "t0", "step", "count", "mode", "out", "stream"]
    bad = [dict(img=None), dict(mot=None), dict(out=None), dict(count=0), dict(count=-5), dict(step=2), dict(step=0),
           dict(t0=2), dict(t0=-1), dict(t0=4), dict(t0=1, step=-1), dict(t=0), dict(mode=2),
           dict(mode=_lib.TRACK_FORCE_STEPS | 2), dict(mode=0x400),
           dict(mode=_lib.TRACK_FORCE_STEPS | _lib.TRACK_FORCE_LDS), dict(n=0), dict(c=-1), dict(h=0), dict(w=0),
           dict(out=P(0x10000)), dict(out=P(0x10000 - 4)), dict(out=P(0x10000 + 2 * 2 * 5 * 9 * 4 - 4))]
    for change in bad:
        a = dict(ok, **change)
        assert lib.clasfv_track(*[a[k] for k in order]) == EINVAL, change
        assert lib.clasfv_last_error(), change
    for change in (dict(h=65536, w=32768), dict(n=65536, c=32768)):
        a = dict(ok, **change)
        assert lib.clasfv_track(*[a[k] for k in order]) == EBADSHAPE, change


def test_warp_overlap_refusals_need_no_gpu():
    """clasfv_warp refuses an out that overlaps img or motion, clasfv_warp_backward a gradient that overlaps
    an input or the other gradient: CLASFV_EINVAL with a message, before any HIP call (the pointers here are
    never dereferenced). motion's range runs from its first to its last element under the strides given, so
    an out between the planes of a strided slice is refused. These pointers are made up, and a call that passed
    the checks would launch on them, so the test runs only where no GPU is visible; where there is one, the
    same refusals and the calls that pass, adjacent buffers among them, run on real tensors in
    tests/test_track_gpu.py."""
    import torch
    from clasfv_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: made-up pointers are handed to the library only where nothing can launch")
    lib = _lib.load()
    P = ctypes.c_void_p
    n, c, h, w = 2, 2, 5, 9
    img_b, hw = n * c * h * w * 4, h * w * 4
    IMG, MOT, OUT, G1, G2 = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    sn, sc = 12 * h * w, 3 * h * w     # the slice [:, 2:, t] of a (n,4,3,h,w) field: it spans 16 planes
    span = 16 * hw

    def warp(out, img=IMG, mot=MOT, m_sn=sn, m_sc=sc):
        return lib.clasfv_warp(P(img), n, c, h, w, P(mot), m_sn, m_sc, P(out), None)

    for out, why in ((IMG, "img"), (IMG + img_b - 4, "img"), (IMG - img_b + 4, "img"), (MOT, "motion"),
                     (MOT + span - 4, "motion"), (MOT - img_b + 4, "motion"), (MOT + 4 * hw, "motion")):
        assert warp(out) == EINVAL, hex(out)
        assert f"out overlaps {why}".encode() in lib.clasfv_last_error(), hex(out)
    assert warp(MOT + 2 * hw, m_sn=2 * h * w, m_sc=-h * w) == EINVAL        # a negative channel stride reaches back
    assert warp(MOT - img_b - hw + 4, m_sn=2 * h * w, m_sc=-h * w) == EINVAL

    def backward(gimg=G1, gmot=G2, gout=OUT):
        return lib.clasfv_warp_backward(P(gout), P(IMG), n, c, h, w, P(MOT), sn, sc, P(gimg) if gimg else None,
                                        P(gmot) if gmot else None, None)

    for kw, msg in ((dict(gimg=IMG), "grad_img overlaps an input"), (dict(gimg=OUT + 4), "grad_img overlaps an input"),
                    (dict(gimg=MOT + span - 4), "grad_img overlaps an input"),
                    (dict(gmot=IMG + img_b - 4), "grad_motion overlaps an input"),
                    (dict(gmot=MOT), "grad_motion overlaps an input"), (dict(gimg=None, gmot=OUT), "grad_motion overlaps"),
                    (dict(gimg=G1, gmot=G1 + img_b - 4), "grad_img overlaps grad_motion")):
        assert backward(**kw) == EINVAL, kw
        assert msg.encode() in lib.clasfv_last_error(), kw
    assert backward(gimg=None, gmot=None) == EINVAL


def test_track_constants_match_header():
    from clasfv_amd import _lib
    defs = {k: int(v, 0) for k, v in re.findall(r"#define CLASFV_TRACK_(\w+)\s+(\w+)", open(HEADER).read())}
    assert defs == {"BILINEAR": _lib.TRACK_BILINEAR, "NEAREST": _lib.TRACK_NEAREST,
                    "FORCE_STEPS": _lib.TRACK_FORCE_STEPS, "FORCE_LDS": _lib.TRACK_FORCE_LDS,
                    "LDS_MAX_PIXELS": _lib.TRACK_LDS_MAX_PIXELS, "LDS_AUTO_PIXELS": _lib.TRACK_LDS_AUTO_PIXELS}
    assert 2 * 4 * _lib.TRACK_LDS_MAX_PIXELS <= 160 * 1024     # two float planes in one CU's LDS
    assert 0 < _lib.TRACK_LDS_AUTO_PIXELS <= _lib.TRACK_LDS_MAX_PIXELS
    assert (_lib.TRACK_FORCE_STEPS | _lib.TRACK_FORCE_LDS) & (_lib.TRACK_BILINEAR | _lib.TRACK_NEAREST) == 0


def test_track_python_checks_need_no_gpu():
    """Shape and mode errors of warp.track / warp.track_labels are raised before the library is called."""
    import torch
    from clasfv_amd import warp as W
    img, mot = torch.zeros(1, 2, 4, 6), torch.zeros(1, 4, 3, 4, 6)
    for args, kw in (((img, mot, 0, 2), dict(mode="cubic")), ((img, mot[:, :2], 0, 2), {}), ((img[0], mot, 0, 2), {}),
                     ((img, mot[..., :5], 0, 2), {}), ((torch.zeros(2, 2, 4, 6), mot, 0, 2), {})):
        with pytest.raises(ValueError):
            W.track(*args, **kw)
    lab = torch.zeros(1, 3, 4, 6, dtype=torch.int64)
    for args in ((lab.float(), mot, 0), (lab, mot, 3), (lab, mot, -1), (lab[0], mot, 0), (lab, mot[:, :, :2], 0)):
        with pytest.raises(ValueError):
            W.track_labels(*args)


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "src", "visualization_utils.py")),
                    reason="the reference checkout is not on this machine")
def test_track_golden_regenerates_identically(tmp_path):
    out = str(tmp_path / "track.npz")
    script = os.path.join(REPO, "tests", "golden", "make_golden_track.py")
    r = subprocess.run([sys.executable, script, "--out", out], capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    new, old = np.load(out, allow_pickle=False), golden("track.npz")
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
