"""What the Python surface refuses before it calls the library.

The C ABI takes raw pointers and a few integers and cannot know what the pointers point at, so the wrappers
are the only place where a tensor's device, dtype, shape and length can be checked. One table of bad calls
runs twice: with every tensor on the host (no GPU needed) and with device tensors (``gpu``). In both runs the
library is replaced by a stub whose every attribute fails the test with "reached the library", and taking a
pointer or a stream for the ABI fails the same way: no case here can launch a kernel, whatever the wrapper
does, which is what makes the table safe to run against wrappers that are wrong. There is deliberately no
variant of these cases that lets a bad call through to the real library; the valid neighbours of every
refusal run in tests/test_abi_audit_gpu.py.

Each case must raise ValueError (TypeError for a non-tensor where a tensor is required) whose message names
the offending argument. ``D`` puts a tensor on the run's device and ``Hst`` leaves it on the host, so "a host
tensor where a device tensor is required" is the same case in both runs; in the host run every tensor is a
host tensor, so there the refusal may name the wrapper's first tensor argument instead.
"""
import re

import numpy as np
import pytest
import torch

T, K, HW = 70, 3, 16   # the plumbing's shapes: three shifted passes of two clips each


class Stub:
    """Stands where the ctypes library does: touching it is the failure the table looks for."""

    def __getattr__(self, name):
        pytest.fail(f"reached the library: {name}")


def _no_pointer(*a, **kw):
    pytest.fail("reached the library: a pointer or stream was taken for the ABI")


@pytest.fixture
def stub(monkeypatch):
    from clasfv_amd import _lib
    s = Stub()
    monkeypatch.setattr(_lib, "load", lambda: s)
    monkeypatch.setattr(_lib, "_lib", s)
    monkeypatch.setattr(_lib, "ptr", _no_pointer)
    monkeypatch.setattr(_lib, "stream_ptr", _no_pointer)
    return s


def engine(stub):
    """An Engine without a handle: forward()'s checks need its device only, and its library is the stub."""
    from clasfv_amd.model import Engine
    e = Engine.__new__(Engine)
    e.lib, e.h, e.device, e.dtype = stub, None, torch.device("cuda", 0), "fp32"
    return e


def Hst(t):
    return t


# ---- the table: (id, wrapper's first tensor argument, argument the refusal names, exception, call(D, stub)) ----
CASES = []


def case(cid, first, arg, call, exc=ValueError):
    CASES.append(pytest.param(first, arg, exc, call, id=cid))


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def _warp_cases():
    from clasfv_amd.warp import warp
    n, c, h, w = 2, 2, 5, 9
    img, mot = (lambda: z(n, c, h, w)), (lambda: z(n, 2, h, w))
    for grad in (False, True):
        tag = "-autograd" if grad else ""
        g = (lambda t: t.requires_grad_()) if grad else (lambda t: t)
        case(f"warp-img-host{tag}", "img", "img", lambda D, s, g=g: warp(Hst(img()), g(D(mot()))))
        case(f"warp-motion-host{tag}", "img", "motion", lambda D, s, g=g: warp(g(D(img())), Hst(mot())))
        for dt in (torch.float64, torch.float16, torch.bfloat16, torch.int64):
            name = str(dt).split(".")[1]
            case(f"warp-img-{name}{tag}", "img", "img",
                 lambda D, s, g=g, dt=dt: warp(D(img().to(dt)), g(D(mot()))))
            case(f"warp-motion-{name}{tag}", "img", "motion",
                 lambda D, s, g=g, dt=dt: warp(g(D(img())), D(mot().to(dt))))
    case("warp-img-not-a-tensor", "img", "img", lambda D, s: warp(np.zeros((n, c, h, w), np.float32), D(mot())), TypeError)
    case("warp-motion-not-a-tensor", "img", "motion", lambda D, s: warp(D(img()), np.zeros((n, 2, h, w), np.float32)),
         TypeError)
    case("warp-out-host", "img", "out", lambda D, s: warp(D(img()), D(mot()), out=Hst(img())))
    case("warp-out-not-a-tensor", "img", "out", lambda D, s: warp(D(img()), D(mot()), out=np.zeros((n, c, h, w), np.float32)),
         TypeError)

    def out_is_img(D, s):
        i = D(img())
        warp(i, D(mot()), out=i)

    def out_in_motion(D, s):
        buf = D(z(n * 2 * h * w + h * w))   # motion at its start, out one plane further: they share all but a plane
        warp(D(img()), buf[:n * 2 * h * w].view(n, 2, h, w), out=buf[h * w:].view(n, c, h, w))

    def out_in_motion_slice(D, s):
        field = D(z(n, 4, 3, h, w))          # the slice's span runs to its last plane, across the gaps between
        out = field.view(-1)[(2 * 3 + 2) * h * w:][:n * c * h * w].view(n, c, h, w)
        warp(D(img()), field[:, 2:, 1], out=out)

    case("warp-out-is-img", "img", "out", out_is_img)
    case("warp-out-overlaps-motion", "img", "out", out_in_motion)
    case("warp-out-inside-a-motion-slice", "img", "out", out_in_motion_slice)


def _track_cases():
    from clasfv_amd import warp as W
    from clasfv_amd.echo import lv_curve
    from clasfv_amd.render import annotate_video
    img, mot = (lambda: z(2, 2, 5, 9)), (lambda: z(2, 4, 4, 5, 9))
    case("track-img-host", "img", "img", lambda D, s: W.track(Hst(img()), D(mot()), 0, 3))
    case("track-motion-host", "img", "motion", lambda D, s: W.track(D(img()), Hst(mot()), 0, 3))
    case("track_labels-labels-host", "labels", "labels",
         lambda D, s: W.track_labels(Hst(z(2, 4, 5, 9, dtype=torch.int64)), D(mot()), 1))
    case("track_labels-motion-host", "labels", "motion",
         lambda D, s: W.track_labels(D(z(2, 4, 5, 9, dtype=torch.int64)), Hst(mot()), 1))
    case("lv_curve-masks-host", "masks", "masks", lambda D, s: lv_curve(Hst(z(3, 8, 8, dtype=torch.uint8))))
    vid, msk = (lambda: z(3, 2, 8, 8)), (lambda: z(2, 8, 8, dtype=torch.uint8))
    case("annotate_video-video-host", "video", "video", lambda D, s: annotate_video(Hst(vid()), D(msk()), size=8))
    case("annotate_video-masks-host", "video", "masks", lambda D, s: annotate_video(D(vid()), Hst(msk()), size=8))
    case("annotate_video-truth-host", "video", "truth",
         lambda D, s: annotate_video(D(vid()), D(msk()), truth=Hst(msk()), size=8))


def _normalize_cases():
    from clasfv_amd.preprocess import zeroone_normalize_
    case("zeroone_normalize_-host", "video", "video", lambda D, s: zeroone_normalize_(Hst(z(3, 4, 8, 8))))
    case("zeroone_normalize_-not-a-tensor", "video", "video",
         lambda D, s: zeroone_normalize_(np.zeros((3, 4, 8, 8), np.float32)), TypeError)


def _plumbing_cases():
    from clasfv_amd import fuse_utils as FU
    table, clip0 = FU.clip_table(T, K, 1, True)
    assert clip0 == [0, 2, 4] and len(table) == 6
    vid = lambda: z(3, T, HW, HW)
    logits = lambda n=6: z(n, 2, 32, HW, HW)

    case("build_clips-video-host", "video_dev", "video_dev", lambda D, s: FU.build_clips(Hst(vid()), table))
    case("build_clips-not-a-tensor", "video_dev", "video_dev",
         lambda D, s: FU.build_clips(np.zeros((3, T, HW, HW), np.float32), table), TypeError)
    # T = 70: an interpolated pass of T_k frames with T_k % 32 != 0 has 32 * n_clips(T_k) frames, any other T_k
    for cid, tab, interp in (("shift-is-T", [(T, 0)], True), ("shift-negative", [(0, 0), (-1, 0)], True),
                             ("first-negative", [(0, -1)], True),
                             ("first-past-the-resampled-pass", [(0, 0), (0, 33)], True),           # 33 + 32 > 64
                             ("first-past-the-resampled-shifted-pass", [(22, 33)], True),           # T_k = 48 -> 64
                             ("first-past-a-whole-pass", [(6, 33)], True),                          # T_k = 64
                             ("first-past-the-raw-pass", [(0, 39)], False),                         # 39 + 32 > 70
                             ("first-past-the-raw-shifted-pass", [(2, 37)], False)):                # 37 + 32 > 68
        case(f"build_clips-{cid}", "video_dev", "table",
             lambda D, s, tab=tab, interp=interp: FU.build_clips(D(vid()), tab, interp))

    case("logit_margin-host", "logits", "logits", lambda D, s: FU.logit_margin(Hst(logits())))
    case("logit_margin-not-a-tensor", "logits", "logits", lambda D, s: FU.logit_margin(logits().numpy()), TypeError)

    case("pass_labels-host", "logits", "logits", lambda D, s: FU.pass_labels(Hst(logits()), clip0, T, 1))
    case("pass_labels-margin-host", "logits", "logits",
         lambda D, s: FU.pass_labels(Hst(z(6, 32, HW, HW)), clip0, T, 1, margin=True))
    case("pass_labels-not-a-tensor", "logits", "logits", lambda D, s: FU.pass_labels(logits().numpy(), clip0, T, 1),
         TypeError)
    case("pass_labels-rank-4", "logits", "logits", lambda D, s: FU.pass_labels(D(z(6, 2, 32, HW)), clip0, T, 1))
    case("pass_labels-rank-6", "logits", "logits", lambda D, s: FU.pass_labels(D(z(1, 6, 2, 32, HW, HW)), clip0, T, 1))
    case("pass_labels-margin-rank-5", "logits", "logits",
         lambda D, s: FU.pass_labels(D(logits()), clip0, T, 1, margin=True))
    case("pass_labels-three-classes", "logits", "logits", lambda D, s: FU.pass_labels(D(z(6, 3, 32, HW, HW)), clip0, T, 1))
    case("pass_labels-16-frames", "logits", "logits", lambda D, s: FU.pass_labels(D(z(6, 2, 16, HW, HW)), clip0, T, 1))
    case("pass_labels-margin-16-frames", "logits", "logits",
         lambda D, s: FU.pass_labels(D(z(6, 16, HW, HW)), clip0, T, 1, margin=True))
    case("pass_labels-five-clips-of-six", "logits", "logits", lambda D, s: FU.pass_labels(D(logits(5)), clip0, T, 1))
    case("pass_labels-margin-five-clips-of-six", "logits", "logits",
         lambda D, s: FU.pass_labels(D(z(5, 32, HW, HW)), clip0, T, 1, margin=True))
    case("pass_labels-clip0-past-the-end", "logits", "logits", lambda D, s: FU.pass_labels(D(logits()), [0, 2, 5], T, 1))
    case("pass_labels-clip0-negative", "logits", "clip0", lambda D, s: FU.pass_labels(D(logits()), [0, -2, 4], T, 1))

    labels = lambda k=K: z(k, 12, HW, HW, dtype=torch.uint8)
    case("fuse_votes-host", "labels", "labels", lambda D, s: FU.fuse_votes(Hst(labels()), 1))
    case("fuse_votes-not-a-tensor", "labels", "labels", lambda D, s: FU.fuse_votes(labels().numpy(), 1), TypeError)
    case("fuse_votes-rank-3", "labels", "labels", lambda D, s: FU.fuse_votes(D(labels()[0]), 1))
    case("fuse_votes-rank-5", "labels", "labels", lambda D, s: FU.fuse_votes(D(labels()[None]), 1))
    case("fuse_votes-step-0", "labels", "step", lambda D, s: FU.fuse_votes(D(labels()), 0))
    case("fuse_votes-step-negative", "labels", "step", lambda D, s: FU.fuse_votes(D(labels()), -1))
    case("fuse_votes-step-leaves-no-frame", "labels", "step", lambda D, s: FU.fuse_votes(D(labels()), 13))
    case("fuse_votes-65-passes", "labels", "labels", lambda D, s: FU.fuse_votes(D(z(65, 2, 4, 4, dtype=torch.uint8)), 1))


def _forward_cases():
    n, t, h, w = 1, 8, 16, 16
    x, seg, mot = (lambda: z(n, 3, t, h, w)), (lambda: z(n, 2, t, h, w)), (lambda: z(n, 4, t, h, w))
    fwd = lambda s, a, b, c: engine(s).forward(a, b, c)
    case("forward-x-host", "x", "x", lambda D, s: fwd(s, Hst(x()), D(seg()), D(mot())))
    case("forward-seg-host", "x", "seg", lambda D, s: fwd(s, D(x()), Hst(seg()), D(mot())))
    case("forward-mot-host", "x", "mot", lambda D, s: fwd(s, D(x()), D(seg()), Hst(mot())))
    case("forward-x-not-a-tensor", "x", "x", lambda D, s: fwd(s, x().numpy(), D(seg()), D(mot())), TypeError)
    bad_x = {"float64": x().double(), "float16": x().half(), "two-channels": z(n, 2, t, h, w), "rank-4": x()[0],
             "transposed": x().transpose(3, 4)}
    for cid, bx in bad_x.items():
        case(f"forward-x-{cid}", "x", "x", lambda D, s, bx=bx: fwd(s, D(bx), D(seg()), D(mot())))
    # sliced after the move: a copy to another device would come out dense
    case("forward-x-strided", "x", "x", lambda D, s: fwd(s, D(z(n, 3, t, h, 2 * w))[..., ::2], D(seg()), D(mot())))
    case("forward-seg-strided", "x", "seg", lambda D, s: fwd(s, D(x()), D(z(n, 2, t, h, 2 * w))[..., ::2], D(mot())))
    case("forward-mot-strided", "x", "mot", lambda D, s: fwd(s, D(x()), D(seg()), D(z(n, 4, t, h, 2 * w))[..., ::2]))
    for name, good, ch in (("seg", seg, 2), ("mot", mot, 4)):
        bad = {"float64": good().double(), "bfloat16": good().bfloat16(), "other-channels": z(n, 6 - ch, t, h, w),
               "other-frames": z(n, ch, t + 8, h, w), "other-batch": z(n + 1, ch, t, h, w), "flat": good().view(-1),
               "transposed": good().transpose(3, 4)}
        for cid, b in bad.items():
            if name == "seg":
                case(f"forward-seg-{cid}", "x", "seg", lambda D, s, b=b: fwd(s, D(x()), D(b), D(mot())))
            else:
                case(f"forward-mot-{cid}", "x", "mot", lambda D, s, b=b: fwd(s, D(x()), D(seg()), D(b)))
    vox = t * h * w

    def seg_in_mot(D, s):
        buf = D(z(n * 5 * vox))   # seg's second plane is mot's first
        fwd(s, D(x()), buf[:n * 2 * vox].view(n, 2, t, h, w), buf[n * vox:].view(n, 4, t, h, w))

    def seg_in_x(D, s):
        buf = D(z(n * 4 * vox))
        fwd(s, buf[:n * 3 * vox].view(n, 3, t, h, w), buf[n * 2 * vox:].view(n, 2, t, h, w), D(mot()))

    def mot_in_x(D, s):
        buf = D(z(n * 6 * vox))
        fwd(s, buf[:n * 3 * vox].view(n, 3, t, h, w), D(seg()), buf[n * 2 * vox:].view(n, 4, t, h, w))

    case("forward-seg-overlaps-mot", "x", "seg", seg_in_mot)
    case("forward-seg-overlaps-x", "x", "seg", seg_in_x)
    case("forward-mot-overlaps-x", "x", "mot", mot_in_x)


_warp_cases()
_track_cases()
_normalize_cases()
_plumbing_cases()
_forward_cases()


def refused(first, arg, exc, call, D, stub, host_run):
    with pytest.raises(exc) as e:
        call(D, stub)
    assert type(e.value) is exc, f"{type(e.value).__name__} where {exc.__name__} is the contract: {e.value}"
    names = {arg, first} if host_run else {arg}
    assert any(re.search(rf"\b{re.escape(nm)}\b", str(e.value)) for nm in names), \
        f"the refusal names none of {sorted(names)}: {e.value}"


@pytest.mark.parametrize("first,arg,exc,call", CASES)
def test_refused_on_the_host(first, arg, exc, call, stub):
    """Every tensor on the host: each case is refused before the library, a pointer or a stream is touched."""
    refused(first, arg, exc, call, lambda t: t, stub, host_run=True)


@pytest.mark.gpu
@pytest.mark.parametrize("first,arg,exc,call", CASES)
def test_refused_on_the_device(first, arg, exc, call, stub):
    """Device tensors (and the one host tensor of a case): the refusal names the argument that is wrong."""
    dev = torch.device("cuda", 0)
    refused(first, arg, exc, call, lambda t: t.to(dev), stub, host_run=False)


def test_clip_table_is_checked_on_a_cache_miss_only(stub, monkeypatch):
    """The table's host list is validated where it is uploaded: a cached table costs the hot path nothing, and
    its key holds the frame count and the interpolation flag it was checked for."""
    from clasfv_amd import fuse_utils as FU
    seen = []
    real = FU.check_clip_table
    monkeypatch.setattr(FU, "check_clip_table", lambda *a: (seen.append(a), real(*a)))
    monkeypatch.setattr(FU, "_TABLES", {})

    class Tab:   # stands for the uploaded tensor: the cache only records the stream on it
        device = None

        def record_stream(self, s):
            pass

    from types import SimpleNamespace
    monkeypatch.setattr(FU, "torch", SimpleNamespace(tensor=lambda *a, **kw: Tab(),
                                                     cuda=SimpleNamespace(current_stream=lambda d=None: None)))
    table = [(0, 0), (0, 32), (1, 0)]
    a = FU._device_table(table, "cuda:0", 70, True)
    assert FU._device_table(table, "cuda:0", 70, True) is a and len(seen) == 1
    assert FU._device_table(table, "cuda:0", 96, True) is not a and len(seen) == 2      # another video length
    assert FU._device_table(table, "cuda:0", 70, False) is not a and len(seen) == 3     # the other rule
    with pytest.raises(ValueError, match="table"):
        FU._device_table([(0, 40)], "cuda:0", 70, True)
    assert len(FU._TABLES) == 3, "a refused table is not cached"


def test_check_clip_table_accepts_every_table_the_package_builds():
    """No refusal of what clip_table makes, for every video length, pass count and step the plumbing meets."""
    from clasfv_amd import fuse_utils as FU
    for t in list(range(33, 140)) + [199, 200, 256]:
        for f, step in ((1, 1), (5, 1), (3, 2), (10, 1), (5, 3)):
            k = FU.clamp_num_clips(t, f, step, strict_reference=False)
            FU.check_clip_table(FU.clip_table(t, k, step, True)[0], t, True)
    for t in (64, 96):
        FU.check_clip_table(FU.clip_table(t, 1, 1, False)[0], t, False)


def test_plumbing_argument_checks_on_shapes_alone():
    """The length, rank and integer checks of pass_labels and fuse_votes are host arithmetic on a shape: each
    refusal of the table above, and its valid neighbour, without a tensor (in the host run of the table a
    host tensor is refused for being one before these checks are reached)."""
    from clasfv_amd import fuse_utils as FU
    clip0, hw = [0, 2, 4], (HW, HW)
    ok = (6, 2, 32) + hw
    assert FU.check_pass_labels_args(ok, clip0, T, 1) == 6
    assert FU.check_pass_labels_args((9,) + ok[1:], clip0, T, 1) == 6            # more clips than needed is fine
    assert FU.check_pass_labels_args((6, 32) + hw, clip0, T, 1, margin=True) == 6
    assert FU.check_pass_labels_args(ok, clip0, T, 2) == 6                        # 70, 68, 66 frames: two clips each
    assert FU.check_pass_labels_args((5, 2, 32) + hw, [0, 2, 3], 70, 11) == 5     # 70, 59, 48 (1.5 -> 2, half to even)
    assert FU.check_pass_labels_args((1, 2, 32) + hw, [0], 32, 1) == 1
    bad = [((5, 2, 32) + hw, clip0, T, 1, False, "logits"), ((5, 32) + hw, clip0, T, 1, True, "logits"),
           (ok, [0, 2, 5], T, 1, False, "logits"), (ok, [0, -2, 4], T, 1, False, "clip0"),
           (ok, [0, 2.5, 4], T, 1, False, "clip0"), ((6, 2, 32, HW), clip0, T, 1, False, "logits"),
           ((1,) + ok, clip0, T, 1, False, "logits"), (ok, clip0, T, 1, True, "logits"),
           ((6, 3, 32) + hw, clip0, T, 1, False, "logits"), ((6, 2, 16) + hw, clip0, T, 1, False, "logits"),
           ((6, 16) + hw, clip0, T, 1, True, "logits"), (ok, clip0, 0, 1, False, "t ="), (ok, clip0, 65536, 1, False, "t ="),
           (ok, clip0, 2 ** 32 + T, 1, False, "t ="), (ok, clip0, T, 0, False, "step"), (ok, clip0, T, 35, False, "step"),
           (ok, clip0, 70.5, 1, False, "t ="), (ok, list(range(65)), T, 1, False, "clip0")]
    for shape, c0, t, step, margin, name in bad:
        with pytest.raises(ValueError, match=re.escape(name)):
            FU.check_pass_labels_args(shape, c0, t, step, margin)
    for shape, step in (((3, 12) + hw, 1), ((3, 12) + hw, 12), ((64, 2, 4, 4), 1), ((1, 1, 1, 1), 1)):
        FU.check_fuse_votes_args(shape, step)
    for shape, step, name in (((12,) + hw, 1, "labels"), ((1, 3, 12) + hw, 1, "labels"), ((65, 2, 4, 4), 1, "labels"),
                              ((0, 2, 4, 4), 1, "labels"), ((3, 12) + hw, 0, "step"), ((3, 12) + hw, -1, "step"),
                              ((3, 12) + hw, 13, "step"), ((3, 12) + hw, 1.5, "step"), ((3, 12) + hw, 2 ** 32 + 1, "step")):
        with pytest.raises(ValueError, match=name):
            FU.check_fuse_votes_args(shape, step)
