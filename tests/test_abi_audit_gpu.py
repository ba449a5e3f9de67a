"""Every public entry point of the package, once, under tests/abi_audit.py's AuditedLib: each call that
reaches libclasfv.so is held against the footprint the header gives it -- live allocations, extents,
alignment, overlap, integer ranges, the stream -- before it is forwarded. The shapes are the smallest the
entry points take; the inputs reach the wrappers' non-trivial paths (strided tensors, a view at a 4-byte
storage offset where the header allows any float alignment, a motion slice of a 5-D field, autograd with its
backward chains, out=, both SIMPLE kernels, margins, strict_reference=False, an empty track range) and are the
valid neighbours of the refusals in tests/test_surface_refusals.py, so a check that refuses too much fails
here. Every input is valid, so nothing is launched that the package does not launch anyway.

The audit's own checks are tested on the host (no GPU) against a recording stand-in for the library.
"""
import ctypes
from collections import Counter

import numpy as np
import pytest
import torch

from tests import abi_audit as A
from tests.golden.fake_model import fake_model

gpu = pytest.mark.gpu
T, K, HW = 70, 3, 16


def dev():
    return torch.device("cuda", 0)


def D(a):
    return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(dev())


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def offset4(t):
    """The same values in a contiguous view that starts 4 bytes into its storage (4 bytes or fewer per element)."""
    assert t.element_size() <= 4
    n = 4 // t.element_size()
    buf = torch.empty(t.numel() + n, dtype=t.dtype, device=t.device)
    buf[n:] = t.reshape(-1)
    v = buf[n:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 and v.storage_offset() == n
    return v


def strided(t):
    """The same values with the last axis at stride 2."""
    big = torch.empty(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    v = big[..., ::2]
    v.copy_(t)
    assert not v.is_contiguous() or t.shape[-1] == 1
    return v


_MODELS = {}


def model_of(dtype):
    if dtype not in _MODELS:
        from clasfv_amd.model import R2plus1D_18_MotionNet
        _MODELS[dtype] = R2plus1D_18_MotionNet(pretrained=False, dtype=dtype)
    return _MODELS[dtype]


# ---- the scenarios: f(aud, monkeypatch); every one ends synchronised ---------------------------------------
def forward(dtype):
    def run(aud, mp):
        m = model_of(dtype)
        mp.setattr(m.engine, "lib", aud)
        r = rng(1)
        x1 = offset4(D(r.uniform(0, 1, (1, 3, 8, 16, 16)).astype(np.float32)))     # pack_input reads x by the float
        x2 = D(r.uniform(0, 1, (2, 8, 3, 16, 32)).astype(np.float32)).permute(0, 2, 1, 3, 4)
        assert not x2.is_contiguous()
        for x in (x1, x2):
            seg, mot = m(x)
            assert seg.shape == (x.shape[0], 2) + x.shape[2:] and mot.shape == (x.shape[0], 4) + x.shape[2:]
        seg_h, _ = m(x1.cpu().numpy())                       # host input is documented: uploaded, then the same call
        assert torch.equal(seg_h, m(x1)[0])
        xc = x2.contiguous()
        seg = torch.empty((2, 2, 8, 16, 32), device=dev())
        mot = torch.empty((2, 4, 8, 16, 32), device=dev())
        m.engine.forward(xc, seg, mot)                        # preallocated buffers, as bench.py uses it
        assert torch.equal(seg, m(x2)[0])
        torch.cuda.synchronize()
        assert aud.calls["clasfv_forward"] == 6
    return run


def plumbing(step):
    def run(aud, mp):
        from clasfv_amd import fuse_utils as FU
        r = rng(2 + step)
        video = strided(D(r.uniform(0, 1, (3, T, HW, HW)).astype(np.float32)))
        table, clip0 = FU.clip_table(T, K, step, True)
        clips = FU.build_clips(video, table)
        assert clips.shape == (len(table), 3, 32, HW, HW)
        assert torch.equal(FU.build_clips(video.double(), table), clips)      # converted, as documented
        logits = fake_model(clips)[0]
        need = max(c + FU.n_clips(T - k * step) for k, c in enumerate(clip0))
        assert need == logits.shape[0]                                         # exactly the clips the passes read
        labels = FU.pass_labels(logits, clip0, T, step)
        margin = FU.logit_margin(offset4(logits.contiguous()))                 # float alignment only: the scalar path
        assert torch.equal(margin, FU.logit_margin(strided(logits)))
        by_margin = FU.pass_labels(margin, clip0, T, step, margin=True)
        for k in range(K):
            assert torch.equal(labels[k, :T - k * step], by_margin[k, :T - k * step])
        fused = FU.fuse_votes(labels, step, "simple")                          # K <= 16: the packed kernel
        assert fused.shape == (T - (step - 1), HW, HW)
        assert torch.equal(fused, FU.fuse_votes(strided(labels), step, "simple", force_generic=True))
        for method in ("majority", "staple", "itkvoting"):
            FU.fuse_votes(labels.to(torch.int64), step, method)
        # the valid neighbours of the refused tables: the last clip that fits, resampled and raw
        FU.build_clips(video, [(0, 32), (22, 32), (6, 32)])
        FU.build_clips(video, [(0, 38), (2, 36)], interpolate_last=False)
        short = D(r.uniform(0, 1, (3, 64, HW, HW)).astype(np.float32))
        t64, c64 = FU.clip_table(64, 1, 1, False)
        FU.pass_labels(fake_model(FU.build_clips(short, t64, False))[0], c64, 64, 1, interpolate_last=False)
        assert FU.divide_to_consecutive_clips(short.cpu().numpy()).shape == (2, 3, 32, HW, HW)
        FU.fuse_votes(labels[:, :12], 12, "majority")                          # T' = 1
        FU.fuse_votes(D(r.integers(0, 2, (64, T, 4, 4)).astype(np.uint8)), 1, "simple")   # K = 64: generic
        host = video.cpu().numpy()
        strict = FU.segment_a_video_with_fusion(host, fake_model, step=step, num_clips=K)
        loose = FU.segment_a_video_with_fusion(host, fake_model, step=step, num_clips=K, strict_reference=False)
        assert strict.shape[0] == T - (step - 1) and loose.shape[0] == T
        one = FU.segment_a_video_with_fusion(host[:, :32], fake_model, strict_reference=False)   # K == 0 clamped to 1
        assert one.shape == (32, HW, HW)
        torch.cuda.synchronize()
    return run


def preprocess(aud, mp):
    from clasfv_amd import preprocess as P
    frames = rng(5).integers(0, 256, (5, 7, 9, 3), dtype=np.uint8)
    a = P.preprocess_video(frames, 16, 16)
    assert a.shape == (3, 5, 16, 16)
    assert torch.equal(a, P.preprocess_video(strided(D(frames)), 16, 16))
    raw = P.preprocess_video(torch.from_numpy(frames), 16, 16, normalize=False)
    assert torch.equal(P.zeroone_normalize_(raw.clone()), a)
    host = raw.cpu()
    arr = host.numpy().copy()
    assert P.zeroone_normalizer(host) is host                  # a host tensor: the numpy way, in place
    assert np.array_equal(P.zeroone_normalizer(arr), host.numpy()) and np.array_equal(host.numpy(), a.cpu().numpy())
    dv = raw.clone()
    assert P.zeroone_normalizer(dv) is dv and torch.equal(dv, a)
    half = P.zeroone_normalizer(raw.cpu().to(torch.bfloat16))   # no numpy form: widened, a new float32 tensor
    assert half.dtype == torch.float32 and not half.is_cuda and float(half.min()) == 0.0 and float(half.max()) == 1.0
    torch.cuda.synchronize()
    assert aud.calls["clasfv_zeroone_normalize"] == 7 and aud.calls["clasfv_preprocess_video"] == 3


def warp_and_track(aud, mp):
    from clasfv_amd import warp as W
    n, c, h, w, t = 2, 2, 5, 9, 4
    r = rng(6)
    img = D(r.standard_normal((n, c, h, w)).astype(np.float32))
    field = D(np.tanh(r.normal(0, 0.4, (n, 4, t, h, w))).astype(np.float32))
    aud.register(img, field)   # track's motion pointer is computed by hand: _lib.ptr never sees the field
    base = W.warp(img, field[:, 2:, 1])                        # a slice of the 5-D field, read in place
    assert torch.equal(base, W.warp(strided(img), field[:, 2:, 1].contiguous()))
    out = torch.full_like(img, float("nan"))
    assert W.warp(img, field[:, 2:, 1], out=out) is out and torch.equal(out, base)
    assert torch.equal(W.warp(img, img), W.warp(img, img.clone()))   # img and motion may be one tensor (C = 2)
    gi, gf = img.clone().requires_grad_(), field.clone().requires_grad_()
    W.warp(gi, gf[:, 2:, 1]).sum().backward()
    assert gi.grad.shape == img.shape and gf.grad.shape == field.shape
    only = img.clone().requires_grad_()
    W.warp(only, field[:, :2, 0]).sum().backward()             # grad_motion NULL
    for fwd, (a, b) in ((True, (0, 3)), (False, (3, 0))):
        for mode in ("bilinear", "nearest"):
            frames = W.track(img, field, a, b, forward=fwd, mode=mode)
            assert frames.shape == (3, n, c, h, w)
        gi, gf = img.clone().requires_grad_(), field.clone().requires_grad_()
        W.track(gi, gf, a, b, forward=fwd).sum().backward()   # the _Track chain: one warp_backward per step
        assert gi.grad is not None and gf.grad is not None
    assert W.track(img, field, 2, 2).shape == (0, n, c, h, w)  # an empty range: no call
    W.track(strided(img), strided(field), 0, 4)
    assert torch.equal(W.apply_sequence_deformation(img, field, 1, 1), img)
    W.apply_sequence_deformation(img, field, 3, 1, forward=False, grid_mode="nearest")
    lab = D(r.integers(0, 3, (n, t, h, w)))
    assert W.track_labels(lab, field, 1).shape == (n, t, h, w)
    torch.cuda.synchronize()
    assert aud.calls["clasfv_warp_backward"] == 2 + 3 + 3


def curves_and_video(aud, mp):
    from clasfv_amd import echo, render
    t, h, w = 5, 7, 9
    r = rng(7)
    yy, xx = np.mgrid[0:h, 0:w]
    masks = np.stack([(((yy - 3) / (1.5 + 0.3 * i)) ** 2 + ((xx - 4) / 3.0) ** 2 <= 1) for i in range(t)]).astype(np.uint8)
    m8 = offset4(D(masks))                                     # masks_dev needs no alignment
    curve = echo.lv_curve(m8)
    assert curve.area.shape == (t,) and curve.geom.shape == (t, 12)
    wide = D(masks.astype(np.int64))[None].expand(2, t, h, w).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not wide.is_contiguous()
    assert torch.equal(echo.lv_curve(wide).area[0], curve.area)
    video = D(r.uniform(0, 1, (3, t, h, w)).astype(np.float32))
    kw = dict(size=11, pane_height=20, title_height=3, strip_height=6)
    frames = render.annotate_video(video, m8, **kw)            # the volume pointer computed by hand into lv_curve's rows
    assert frames.shape == (t, 29, 11, 3)
    assert torch.equal(render.annotate_video(strided(video), D(masks.astype(np.int64)), volume=curve.volume, **kw), frames)
    render.annotate_video(video, m8, truth=D(masks[::-1].copy()), title=False, first=1, count=2, **kw)
    render.annotate_video(video, m8, volume=curve.volume.cpu().numpy(), title=np.zeros((3, 11, 3), np.uint8), **kw)
    torch.cuda.synchronize()
    assert aud.calls["clasfv_render_annotated"] == 4 and aud.calls["clasfv_lv_geometry"] == 4


def video_stream(aud, mp):
    import clasfv_amd.synthetic as S
    from clasfv_amd.stream import VideoStream
    videos = [S.echo_video_uint8(40, 20, 24, seed=i, period=20 + 7 * i) for i in range(2)]
    vs = VideoStream(fake_model, num_clips=2, height=HW, width=HW)
    out = vs.run(videos, curves=True)
    assert len(out) == 2 and all(m.shape == (40, HW, HW) and c.area.shape == (40,) for m, c in out)
    plain = vs.run(videos)
    assert all(np.array_equal(a, b[0]) for a, b in zip(plain, out))
    torch.cuda.synchronize()


def sharded(aud, mp):
    from clasfv_amd import dist as DI, fuse_utils as FU
    r = rng(9)
    vids = [D(r.uniform(0, 1, (3, tt, HW, HW)).astype(np.float32)) for tt in (40, 70)]
    out = DI.segment_videos_sharded(vids, fake_model, num_clips=2, step=1, fuse_method="simple")
    assert sorted(out) == [0, 1]
    for i, v in enumerate(vids):
        assert torch.equal(out[i], FU.segment_a_video_with_fusion_device(v, fake_model, num_clips=2))
    torch.cuda.synchronize()


def losses(aud, mp):
    import torch.nn.functional as F
    from clasfv_amd import losses as L
    from tests.golden.make_golden_losses import loss_inputs
    d = loss_inputs()
    video, motion = D(d["video"]).requires_grad_(), D(d["motion"]).requires_grad_()
    L.deformation_motion_loss(video, motion).backward()
    assert video.grad is not None and motion.grad is not None
    motion, logits = D(d["motion"]).requires_grad_(), D(d["logits"]).requires_grad_()
    flow, ots = L.motion_seg_loss(d["ed"], d["es"], d["ed_index"], d["es_index"], motion, F.softmax(logits, dim=1),
                                  start=0, end=d["video"].shape[2])
    (flow + ots).backward()
    assert motion.grad is not None and logits.grad is not None
    with torch.no_grad():
        L.deformation_motion_loss(video, motion)
    torch.cuda.synchronize()


SCENARIOS = {"forward-fp32": forward("fp32"), "forward-bf16": forward("bf16"), "plumbing-step1": plumbing(1),
             "plumbing-step2": plumbing(2), "preprocess": preprocess, "warp-track": warp_and_track,
             "lv_curve-annotate_video": curves_and_video, "VideoStream": video_stream,
             "segment_videos_sharded": sharded, "losses": losses}
REACHED = {}   # scenario -> Counter of the exports it reached, in this process


def run_scenario(name, monkeypatch):
    from clasfv_amd import _lib, fuse_utils as FU
    with monkeypatch.context() as mp:
        aud = A.install(mp, _lib)
        mp.setattr(FU, "_TABLES", {})   # every table is checked and uploaded under the audit
        SCENARIOS[name](aud, mp)
        REACHED[name] = aud.calls
        # the allocator's snapshot resolved every pointer: the fallback registry is a weaker audit and would
        # look the same from outside, so the mode is asserted on the torch build the suite runs on
        assert aud.resolver == "allocator snapshot", aud.resolver
    return aud.calls


@gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_entry_points_stay_inside_their_footprint(name, monkeypatch):
    """No violation: the scenario runs to its end (a violation raises before the call is forwarded)."""
    calls = run_scenario(name, monkeypatch)
    assert sum(calls[n] for n in A.FOOTPRINT) > 0, "the scenario reached no audited export"


@gpu
def test_every_footprint_export_is_reached_through_the_python_surface(monkeypatch):
    """Coverage: each export with a rule was called by some scenario (those not yet run in this process run here)."""
    for name in SCENARIOS:
        if name not in REACHED:
            run_scenario(name, monkeypatch)
    total = Counter()
    for calls in REACHED.values():
        total.update(calls)
    missing = [n for n in A.FOOTPRINT if total[n] == 0]
    assert not missing, f"never reached through the Python surface: {missing}"


# ---- host: the exemption list, and the audit's own checks ---------------------------------------------------
def test_every_pointer_taking_export_has_a_rule_or_an_exemption():
    from clasfv_amd import _lib
    takers = {n for n, (_, args) in _lib.SIGNATURES.items() if A.takes_pointer_or_stream(args)}
    assert set(A.FOOTPRINT) <= takers and set(A.EXEMPT) <= takers
    assert not set(A.FOOTPRINT) & set(A.EXEMPT)
    assert takers == set(A.FOOTPRINT) | set(A.EXEMPT), sorted(takers ^ (set(A.FOOTPRINT) | set(A.EXEMPT)))
    data_taking = {"clasfv_forward", "clasfv_build_clips", "clasfv_pass_labels", "clasfv_pass_labels_margin",
                   "clasfv_logit_margin", "clasfv_fuse_votes", "clasfv_warp", "clasfv_warp_backward", "clasfv_track",
                   "clasfv_zeroone_normalize", "clasfv_preprocess_video", "clasfv_lv_geometry", "clasfv_render_annotated"}
    assert set(A.FOOTPRINT) == data_taking
    assert set(A.EXEMPT.values()) <= {"handle", "handle (host data)", "introspection", "diagnostics"}
    # a rule takes the export's parameters, in order
    import inspect
    for name, rule in A.FOOTPRINT.items():
        assert len(inspect.signature(rule).parameters) == 1 + len(_lib.SIGNATURES[name][1]), name


class Recorder:
    """Stands for the ctypes library on the host: records what was forwarded."""

    def __init__(self):
        self.forwarded = []

    def clasfv_zeroone_workspace_bytes(self):
        return 4096

    def __getattr__(self, name):
        return lambda *a: self.forwarded.append(name) or 0


def audited(blocks, stream=0):
    from clasfv_amd import _lib
    rec = Recorder()
    return A.AuditedLib(rec, _lib.SIGNATURES, blocks=blocks, current_stream=stream), rec


P = ctypes.c_void_p


def test_the_audit_refuses_what_it_is_there_to_find():
    """On a recording stand-in with a given list of live blocks: a valid warp is forwarded; a host pointer, an
    extent past the allocation, a strided motion past it, a misaligned pointer, out over img, an integer that
    ctypes would truncate, a NULL and another stream are each refused, with nothing forwarded."""
    n, c, h, w = 2, 2, 5, 9
    img_b, mot_b, out_b = n * c * h * w * 4, n * 2 * h * w * 4, n * c * h * w * 4
    blocks = [(0x10000, img_b, 0), (0x20000, mot_b, 0), (0x30000, out_b, 0), (0x40000, n * 4 * 3 * h * w * 4, 0)]
    ok = [P(0x10000), n, c, h, w, P(0x20000), 2 * h * w, h * w, P(0x30000), P(0)]
    aud, rec = audited(blocks)
    assert aud.clasfv_warp(*ok) == 0 and rec.forwarded == ["clasfv_warp"] and aud.calls["clasfv_warp"] == 1
    # the backward pair of frame 2 of a (2,4,3,h,w) field, in place: ends exactly at the field's end
    field = [P(0x10000), n, c, h, w, P(0x40000 + (2 * 3 + 2) * h * w * 4), 12 * h * w, 3 * h * w, P(0x30000), P(0)]
    assert aud.clasfv_warp(*field) == 0
    bad = {"host pointer": (0, P(0x7f0000000000)), "past the allocation": (1, n + 1),
           "motion strides past the allocation": (6, 2 * h * w + 1), "misaligned": (8, P(0x30002)),
           "out over img": (8, P(0x10000)), "truncated integer": (2, 2 ** 32 + c), "null": (5, None),
           "null as zero": (0, P(0)), "int64 overflow": (7, 2 ** 63), "not an integer": (3, 5.0)}
    for why, (i, v) in bad.items():
        rec.forwarded.clear()
        with pytest.raises(A.Violation):
            aud.clasfv_warp(*(ok[:i] + [v] + ok[i + 1:]))
        assert rec.forwarded == [], why
    other, rec = audited(blocks, stream=0x5000)
    with pytest.raises(A.Violation, match="stream"):
        other.clasfv_warp(*ok)
    assert other.clasfv_warp(*(ok[:-1] + [P(0x5000)])) == 0 and rec.forwarded == ["clasfv_warp"]


def test_the_audit_reads_the_pass_table_and_allows_documented_nulls():
    """pass_labels' extent comes from the host clip0 array and the header's round-half-even clip count; the
    margin form reads half; warp_backward's gradients may be NULL, its other pointers may not."""
    h = w = 16
    clip = 32 * h * w * 4
    labels_b = 3 * 70 * h * w
    arr = (ctypes.c_int32 * 3)(0, 2, 4)
    p0 = ctypes.cast(arr, P)
    for fn, planes in (("clasfv_pass_labels", 2), ("clasfv_pass_labels_margin", 1)):
        aud, rec = audited([(0x100000, 6 * planes * clip, 0), (0x900000, labels_b, 0)])
        assert getattr(aud, fn)(P(0x100000), 3, p0, 70, 1, h, w, 1, P(0x900000), None) == 0
        short, rec = audited([(0x100000, 5 * planes * clip, 0), (0x900000, labels_b, 0)])
        with pytest.raises(A.Violation, match="logits_dev"):
            getattr(short, fn)(P(0x100000), 3, p0, 70, 1, h, w, 1, P(0x900000), None)
        assert rec.forwarded == []
    assert [A.n_clips(t) for t in (16, 17, 48, 70, 80, 81, 112)] == [0, 1, 2, 2, 2, 3, 4]   # half to even
    n, c = 1, 2
    img_b = n * c * h * w * 4
    aud, rec = audited([(0x10000 * i, img_b, 0) for i in range(1, 6)])
    args = [P(0x10000), P(0x20000), n, c, h, w, P(0x30000), 2 * h * w, h * w, P(0x40000), P(0x50000), None]
    assert aud.clasfv_warp_backward(*args) == 0
    assert aud.clasfv_warp_backward(*(args[:9] + [None, P(0x50000), None])) == 0
    with pytest.raises(A.Violation, match="grad_out_dev is NULL"):
        aud.clasfv_warp_backward(*([None] + args[1:]))
    with pytest.raises(A.Violation, match="overlaps"):
        aud.clasfv_warp_backward(*(args[:9] + [P(0x20000), P(0x50000), None]))   # grad_img over img
    aud, rec = audited([(0x10000, 3 * 100 * 4, 0), (0x20000, 4096, 0)])
    assert aud.clasfv_zeroone_normalize(P(0x10000), 100, P(0x20000), None) == 0  # in place: one read-write range
    with pytest.raises(A.Violation, match="workspace_dev"):
        audited([(0x10000, 3 * 100 * 4, 0), (0x20000, 4092, 0)])[0].clasfv_zeroone_normalize(P(0x10000), 100, P(0x20000), None)
