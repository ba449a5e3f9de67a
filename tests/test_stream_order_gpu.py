"""Every entry point is ordered on the caller's stream alone, and returns without waiting for the device.

The rest of the suite launches on the default stream and synchronises after each call, or puts nothing in
front of a call on another stream: a launch that forgot its stream argument, a missing wait of the side
stream, or a hidden host synchronisation passes there. Here every call runs behind a blocker on a
non-default stream whose inputs are still stale when the call is issued (tests/stream_order.py states the
protocol): through the C ABI for every __global__ function of plumbing.hip, track.hip and lvgeom.hip, for
clasfv_forward, and for clasfv_run_conv / clasfv_run_decoder on every kernel name of
tests/test_layers_gpu.py; on two streams at once; and through the Python layer under torch.cuda.stream(S).

Every case prints one STREAM_CASE line (host time of the call, blocker length, wall time); the MI355X log and
the seeded defects this file catches are in profiles/stream_order_mi355x.txt.
"""
import ctypes
import os
import re
import time
import zlib

import numpy as np
import pytest
import torch

from tests import stream_order as SO
from tests import test_plumbing_gpu as TP
from tests.stream_order import Case, dev

gpu = pytest.mark.gpu   # the three coverage / plan checks below need no GPU and carry no mark

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "fully-automated-multi-heartbeat-echocardiography-video-segmentation-and-motion-tracking_amd",
                    "csrc")
GIMG_RTOL, GIMG_ATOL = 1e-5, 1e-6   # test_warp_vs_oracle's bar for grad_img (float atomics)
# Gradients of a chain of warps, run against run: each is a sum over the chain of warp_backward's atomically
# accumulated grad_img, so two runs differ by the reordering of float32 sums. The project's bar for such
# gradients against the CPU oracle is rtol 1e-4 / atol 1e-7, held to 11.276 units of it at the worst
# (tests/test_track_gpu.py GRAD_BAR); two runs that both meet it are within twice that of each other.
CHAIN_RTOL, CHAIN_ATOL = 2 * 11.276 * 1e-4, 2 * 11.276 * 1e-7


def lib():
    from clasfv_amd import _lib
    return _lib.load()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def pair(draw, *key):
    """(buffer, A, A') on the device for one input: two draws of one recipe."""
    a, b = D(draw(rng_for("A", *key))), D(draw(rng_for("A'", *key)))
    assert not torch.equal(a, b)
    return torch.empty_like(a), a, b


def case_of(name, call, inputs, outs=(), **kw):
    bufs, real, stale = zip(*inputs)
    return Case(name, call, bufs, real, stale, outs, **kw)


def int32_array(vals):
    arr = (ctypes.c_int32 * max(1, len(vals)))(*vals)
    return ctypes.cast(arr, ctypes.c_void_p), arr


# ---- plumbing.hip, track.hip, lvgeom.hip through the C ABI --------------------------------------------------
H, W = 8, 12   # H * W % 4 == 0: the vector bodies


def case_build_clips():
    from clasfv_amd import fuse_utils as FU
    t, k = 70, 3
    table, _ = FU.clip_table(t, k, 1, True)
    n = len(table)
    vid = pair(lambda r: r.standard_normal((3, t, H, W)).astype(np.float32), "clips")
    tab_a = D(np.asarray(table, np.int32).reshape(-1))
    tab_b = torch.zeros_like(tab_a)   # the stale table: every clip (shift 0, first frame 0), valid for any pass
    tab = (torch.empty_like(tab_a), tab_a, tab_b)
    out = torch.empty((n, 3, 32, H, W), device=dev())

    def call():
        SO.ok(lib().clasfv_build_clips(ptr(vid[0]), t, H, W, ptr(tab[0]), n, 1, ptr(out), SO.current_ptr()),
              "clasfv_build_clips")
        return [out]
    return case_of("clasfv_build_clips", call, [vid, tab], [out])


def case_pass_labels(margin):
    from clasfv_amd import fuse_utils as FU
    t, step, k = 70, 1, 3
    table, clip0 = FU.clip_table(t, k, step, True)
    n = len(table)
    shape = (n, 32, H, W) if margin else (n, 2, 32, H, W)
    x = pair(lambda r: r.normal(0.0, 2.0, shape).astype(np.float32), "labels", margin)
    lab = torch.empty((k, t, H, W), dtype=torch.uint8, device=dev())
    cp, keep = int32_array(clip0)
    name = "clasfv_pass_labels_margin" if margin else "clasfv_pass_labels"

    def call(keep=keep):
        SO.ok(getattr(lib(), name)(ptr(x[0]), k, cp, t, step, H, W, 1, ptr(lab), SO.current_ptr()), name)
        return [lab]
    return case_of(name, call, [x], [lab])


def case_logit_margin():
    n = 2
    x = pair(lambda r: r.normal(0.0, 2.0, (n, 2, 32, H, W)).astype(np.float32), "margin")
    out = torch.empty((n, 32, H, W), device=dev())

    def call():
        SO.ok(lib().clasfv_logit_margin(ptr(x[0]), n, H, W, ptr(out), SO.current_ptr()), "clasfv_logit_margin")
        return [out]
    return case_of("clasfv_logit_margin", call, [x], [out])


FUSE_K, FUSE_T = 3, 12
# method -> (clasfv_fuse_votes' method argument, the kernel launch_fuse_votes takes for it at K = 3, 8x12: for SIMPLE
# by the launcher's rule as tests/test_plumbing_gpu.py restates it)
FUSE = {"majority": (0, "fuse_majority_kernel"), "itkvoting": (3, "fuse_majority_kernel"),
        "simple": (1, TP._simple_kernel(FUSE_K, H * W, False)), "simple-generic": (1 | 0x100, TP._simple_kernel(FUSE_K, H * W, True)),
        "staple": (2, "fuse_staple_kernel")}
assert {FUSE["simple"][1], FUSE["simple-generic"][1]} == {"fuse_simple_fast_kernel", "fuse_simple_kernel"}


def case_fuse_votes(which):
    k, t, step = FUSE_K, FUSE_T, 1
    method, _ = FUSE[which]
    lab = pair(lambda r: (r.random((k, t, H, W)) < 0.5).astype(np.uint8), "fuse")   # votes in {0, 1}
    out = torch.empty((t - (step - 1), H, W), dtype=torch.uint8, device=dev())

    def call():
        SO.ok(lib().clasfv_fuse_votes(ptr(lab[0]), k, t, step, H, W, method, ptr(out), SO.current_ptr()),
              "clasfv_fuse_votes")
        return [out]
    return case_of(f"clasfv_fuse_votes[{which}]", call, [lab], [out])


def _grad_out(r, shape):
    return (r.integers(-8, 9, shape) / 32.0).astype(np.float32)   # as test_warp_vs_oracle: sums of few, small terms


def case_warp(backward):
    n, c, h, w = 2, 3, 9, 11
    img = pair(lambda r: r.standard_normal((n, c, h, w)).astype(np.float32), "warp-img")
    mot = pair(lambda r: np.tanh(r.normal(0, 0.4, (n, 4, 3, h, w))).astype(np.float32), "warp-mot")
    view = mot[0][:, 2:, 1]   # a strided slice of an (N,4,T,H,W) tensor
    m_sn, m_sc = view.stride(0), view.stride(1)
    assert (view.stride(2), view.stride(3)) == (w, 1)
    if not backward:
        out = torch.empty((n, c, h, w), device=dev())

        def call():
            SO.ok(lib().clasfv_warp(ptr(img[0]), n, c, h, w, ptr(view), m_sn, m_sc, ptr(out), SO.current_ptr()),
                  "clasfv_warp")
            return [out]
        return case_of("clasfv_warp", call, [img, mot], [out])
    gout = pair(lambda r: _grad_out(r, (n, c, h, w)), "warp-gout")
    # grad_img is accumulated into: the caller's zeros are an input (stale: ones)
    gimg = (torch.empty((n, c, h, w), device=dev()), torch.zeros((n, c, h, w), device=dev()),
            torch.ones((n, c, h, w), device=dev()))
    gmot = torch.empty((n, 2, h, w), device=dev())

    def call():
        SO.ok(lib().clasfv_warp_backward(ptr(gout[0]), ptr(img[0]), n, c, h, w, ptr(view), m_sn, m_sc, ptr(gimg[0]),
                                         ptr(gmot), SO.current_ptr()), "clasfv_warp_backward")
        return [gimg[0], gmot]
    return case_of("clasfv_warp_backward", call, [gout, img, mot, gimg], [gmot], close={0: (GIMG_RTOL, GIMG_ATOL)})


TRACK_HW = (24, 20)


def _track_kernel(mode):
    """clasfv_track's choice as include/clasfv.h states it: FORCE_STEPS the step path always, FORCE_LDS the LDS
    path for every plane that fits, else the LDS path up to CLASFV_TRACK_LDS_AUTO_PIXELS."""
    from clasfv_amd import _lib
    hw = TRACK_HW[0] * TRACK_HW[1]
    if mode & _lib.TRACK_FORCE_STEPS:
        return "track_step_kernel"
    limit = _lib.TRACK_LDS_MAX_PIXELS if mode & _lib.TRACK_FORCE_LDS else _lib.TRACK_LDS_AUTO_PIXELS
    return "track_lds_kernel" if hw <= limit else "track_step_kernel"


TRACK_MODES = {name: (mode, _track_kernel(mode)) for name, mode in
               (("bilinear-lds", 0 | 0x200), ("bilinear-steps", 0 | 0x100), ("nearest-lds", 1 | 0x200),
                ("nearest-steps", 1 | 0x100))}
assert {k for _, k in TRACK_MODES.values()} == {"track_lds_kernel", "track_step_kernel"}


def case_track(which):
    n, c, (h, w), t, p = 1, 2, TRACK_HW, 6, 5
    mode, _ = TRACK_MODES[which]
    nearest = which.startswith("nearest")
    img = pair(lambda r: (r.integers(0, 3, (n, c, h, w)) if nearest else r.standard_normal((n, c, h, w)))
               .astype(np.float32), "track-img", nearest)
    mot = pair(lambda r: np.tanh(r.normal(0, 0.4, (n, 4, t, h, w))).astype(np.float32), "track-mot")
    out = torch.empty((p, n, c, h, w), device=dev())
    m = mot[0]

    def call():
        SO.ok(lib().clasfv_track(ptr(img[0]), n, c, h, w, ptr(m), m.stride(0), m.stride(1), m.stride(2), t, 0, 1, p,
                                 mode, ptr(out), SO.current_ptr()), "clasfv_track")
        return [out]
    return case_of(f"clasfv_track[{which}]", call, [img, mot], [out])


def _ellipses(r, f, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((f, h, w), np.uint8)
    for i in range(f):
        cy, cx = h / 2 + r.uniform(-3, 3), w / 2 + r.uniform(-2, 2)
        a, b = r.uniform(5, 12), r.uniform(3, 6)
        out[i] = ((yy - cy) / a) ** 2 + ((xx - cx) / b) ** 2 <= 1
    return out


def case_lv_geometry():
    f, h, w = 5, 31, 17
    masks = pair(lambda r: _ellipses(r, f, h, w), "lv")   # masks in {0, 1}
    area = torch.empty(f, dtype=torch.int32, device=dev())
    geom = torch.empty((f, 12), dtype=torch.float64, device=dev())

    def call():
        SO.ok(lib().clasfv_lv_geometry(ptr(masks[0]), f, h, w, 1, 1.0, 1.0, ptr(area), ptr(geom), SO.current_ptr()),
              "clasfv_lv_geometry")
        return [area, geom]
    return case_of("clasfv_lv_geometry", call, [masks], [area, geom])


def case_preprocess():
    t, hs, ws, h, w = 6, 20, 24, 16, 16
    frames = pair(lambda r: r.integers(0, 256, (t, hs, ws, 3), dtype=np.uint8), "pre")
    out = torch.empty((3, t, h, w), device=dev())

    def call():
        SO.ok(lib().clasfv_preprocess_video(ptr(frames[0]), t, hs, ws, h, w, ptr(out), SO.current_ptr()),
              "clasfv_preprocess_video")
        return [out]
    return case_of("clasfv_preprocess_video", call, [frames], [out])


def case_normalize(key="norm", n=1025):
    """In place; the workspace is the caller's and holds the partial extrema of the last call (of A', when the
    call behind the blocker is issued): the second launch reads what the first wrote there."""
    vid = pair(lambda r: r.standard_normal((3, n)).astype(np.float32), key)
    ws = torch.zeros(int(lib().clasfv_zeroone_workspace_bytes()) // 4, device=dev())

    def call():
        SO.ok(lib().clasfv_zeroone_normalize(ptr(vid[0]), ctypes.c_int64(n), ptr(ws), SO.current_ptr()),
              "clasfv_zeroone_normalize")
        return [vid[0]]
    return case_of(f"clasfv_zeroone_normalize[{key}]", call, [vid])


PLUMBING = {
    "build_clips": case_build_clips,
    "pass_labels": lambda: case_pass_labels(False), "pass_labels_margin": lambda: case_pass_labels(True),
    "logit_margin": case_logit_margin,
    **{f"fuse_votes-{m}": (lambda m=m: case_fuse_votes(m)) for m in FUSE},
    "warp": lambda: case_warp(False), "warp_backward": lambda: case_warp(True),
    **{f"track-{m}": (lambda m=m: case_track(m)) for m in TRACK_MODES},
    "lv_geometry": case_lv_geometry, "preprocess_video": case_preprocess, "zeroone_normalize": case_normalize,
}
# the __global__ functions each case reaches: the one table of these claims (FUSE and TRACK_MODES derive theirs
# from the launchers' rules)
PLUMBING_KERNELS = {
    "build_clips": {"build_clips_kernel"}, "pass_labels": {"pass_labels_kernel"}, "pass_labels_margin": {"pass_labels_kernel"},
    "logit_margin": {"logit_margin_kernel"},
    **{f"fuse_votes-{m}": {k} for m, (_, k) in FUSE.items()},
    "warp": {"warp_kernel"}, "warp_backward": {"warp_backward_kernel"},
    **{f"track-{m}": {k} for m, (_, k) in TRACK_MODES.items()},
    "lv_geometry": {"lv_geometry_kernel"}, "preprocess_video": {"preprocess_video_kernel"},
    "zeroone_normalize": {"minmax_partial_kernel", "normalize_kernel"},
}


@gpu
@pytest.mark.parametrize("which", sorted(PLUMBING))
def test_plumbing_call_behind_a_blocked_stream(which):
    SO.run_behind_blocker(PLUMBING[which]())


def test_cases_reach_every_global_function_of_the_plumbing_files():
    """The kernels the cases above name are exactly the __global__ functions of plumbing.hip, track.hip and
    lvgeom.hip: a new kernel without a case behind the blocker fails here."""
    defined = set()
    for f in ("plumbing.hip", "track.hip", "lvgeom.hip"):
        defined |= set(re.findall(r"__global__.*?void\s+(\w+)", open(os.path.join(CSRC, f)).read()))
    assert len(defined) == 15, sorted(defined)
    assert set(PLUMBING) == set(PLUMBING_KERNELS)
    claimed = set().union(*PLUMBING_KERNELS.values())
    assert claimed == defined, sorted(claimed ^ defined)


# ---- the engine ------------------------------------------------------------------------------------------
_MODELS = {}


def model_of(dtype):
    if dtype not in _MODELS:
        from clasfv_amd.model import R2plus1D_18_MotionNet
        # the "echo" recipe: its masks follow the synthetic video's LV, so two videos give two fused masks
        _MODELS[dtype] = R2plus1D_18_MotionNet(pretrained=False, dtype=dtype, weights="echo")
    return _MODELS[dtype]


SMALL, LARGER = (1, 3, 8, 16, 32), (2, 3, 16, 64, 48)


def case_forward(dtype, shape, key="x", timing=False, fill=False, model=None):
    eng = (model or model_of(dtype)).engine
    n, _, t, h, w = shape
    x = pair(lambda r: r.uniform(0, 1, shape).astype(np.float32), "forward", shape, key)
    seg = torch.empty((n, 2, t, h, w), device=dev())
    mot = torch.empty((n, 4, t, h, w), device=dev())

    def call():
        eng.forward(x[0], seg, mot, stream=torch.cuda.current_stream(dev()))
        return [seg, mot]

    def fill_arena():   # NaN bytes over the whole arena, stream-ordered: the forward rewrites all it reads
        eng.fill_workspace(0xFF, stream=torch.cuda.current_stream(dev()))

    def read_timing():  # documented to wait: called on a synchronised stream only; empties the event pool's use
        assert eng.kernel_timing(cap=64)
    name = f"clasfv_forward[{dtype}-{'x'.join(map(str, shape))}{'-timing' if timing else ''}{'-fill' if fill else ''}-{key}]"
    return case_of(name, call, [x], [seg, mot], between=fill_arena if fill else None,
                   settled=read_timing if timing else None)


def plan_kernels(dtype, shape):
    from clasfv_amd.model import forward_plan
    n, _, t, h, w = shape
    launches = forward_plan(n, t, h, w, dtype)["launches"]
    return launches, {l["kernel"] for l in launches if l["kernel"]}


def test_forward_plans_hold_what_the_engine_cases_are_for():
    """clasfv_forward_plan (host arithmetic) at the two shapes: the small one already has the pack, three
    forks and the join, eight split-K convs with their split_sum_kernel (fp32 engines), the decoder's index
    kernel and the decoder; the larger one adds conv_wino4 and conv_patch32_bf16."""
    for dtype in ("fp32", "bf16"):
        launches, small = plan_kernels(dtype, SMALL)
        kinds = [l["kind"] for l in launches]
        assert kinds.count("pack") == 1 and kinds.count("fork") == 3 and kinds.count("join") == 1
        assert kinds.count("split_sum") == (8 if dtype == "fp32" else 0)   # the bf16 engine splits no conv
        assert kinds.count("dec_index") == 1 and kinds.count("decoder") == 1
        assert any(l["stream"] == 1 for l in launches)
    _, small = plan_kernels("fp32", SMALL)
    _, larger = plan_kernels("fp32", LARGER)
    assert "conv_wino4" in larger - small
    _, small = plan_kernels("bf16", SMALL)
    _, larger = plan_kernels("bf16", LARGER)
    assert "conv_patch32_bf16" in larger - small


ENGINE_CASES = {
    "fp32-small": lambda: case_forward("fp32", SMALL), "bf16-small": lambda: case_forward("bf16", SMALL),
    "fp32-larger": lambda: case_forward("fp32", LARGER), "bf16-larger": lambda: case_forward("bf16", LARGER),
    "fp32-small-kernel-timing": lambda: case_forward("fp32", SMALL, timing=True),
    "fp32-small-filled-arena": lambda: case_forward("fp32", SMALL, fill=True),
}


@gpu
@pytest.mark.parametrize("which", list(ENGINE_CASES))
def test_forward_behind_a_blocked_stream(which):
    """clasfv_forward: the pack, every conv, the split-K sums, the side stream's projections (forked from and
    joined to the caller's stream by events), the decoder's index kernel and the decoder are all behind the
    blocker; with kernel timing on, its event records do not make the call wait; a NaN fill of the arena
    enqueued in front of the forward changes nothing."""
    case = ENGINE_CASES[which]()
    eng = model_of("fp32").engine
    timing = which.endswith("kernel-timing")
    if timing:
        eng.set_kernel_timing(True)
    try:
        SO.run_behind_blocker(case)
    finally:
        if timing:
            SO.sync()
            eng.set_kernel_timing(False)


# ---- clasfv_run_conv and clasfv_run_decoder ------------------------------------------------------------
def conv_kernel_names():
    from tests import test_layers_gpu as TL
    return sorted([("fp32", k) for k in TL.FP32_KERNELS] + [("bf16", k) for k in TL.BF16_KERNELS])


def smallest_case(nt, dtype, kernel):
    """The case of tests/test_layers_gpu.py CASES of this kernel name with the fewest multiply-adds."""
    from tests import test_layers_gpu as TL

    def macs(c):
        e = nt.by_name[c["layer"]]
        n, t, h, w = c["nthw"]
        return n * t * h * w * (e["cin"] + e["cin2"]) * e["cout"] * e["kernel"][0] * e["kernel"][1] * e["kernel"][2]
    return min((c for c in TL.CASES if c["dtype"] == dtype and c["kernel"] == kernel), key=macs)


@gpu
@pytest.mark.parametrize("dtype,kernel", conv_kernel_names(), ids=lambda v: v)
def test_run_conv_behind_a_blocked_stream(dtype, kernel):
    """clasfv_run_conv on the smallest case of every kernel name, with split-K scratch where
    tests/test_layers_gpu.py hands one over (its partial sums are those of the stale input when the call
    is issued). Stale input: a second draw of build_case's recipe."""
    from tests import test_layers_gpu as TL
    nt = TL.net(dtype, "float")
    c = smallest_case(nt, dtype, kernel)
    real = TL.build_case(nt, c)
    stale = TL.build_case(nt, dict(c, kernel=c["kernel"] + "'"))   # case_id seeds the draw: another id, another draw
    e = real["e"]
    n, to_, ho, wo = real["out"]
    numel = n * to_ * ho * wo * e["cout_p"]
    y = torch.empty(numel, dtype=e["out_dtype"], device=dev())
    scratch = None
    if e["kernel"][0] == 3 and ".conv" in c["layer"]:   # as test_layers_gpu.launch
        scratch = torch.zeros(4 * numel, dtype=torch.float32, device=dev())
    inputs = [(torch.empty_like(real[k]), real[k].clone(), stale[k].clone()) for k in ("x", "x2", "res")
              if real[k] is not None]
    by_key = dict(zip([k for k in ("x", "x2", "res") if real[k] is not None], [i[0] for i in inputs]))
    relu = c["relu"][-1]

    def call():
        name = nt.engine.run_conv(e["index"], by_key["x"], c["nthw"], y, x2=by_key.get("x2"), res=by_key.get("res"),
                                  relu=relu, x_c8=c["x_c8"], y_c8=c["y_c8"], scratch=scratch,
                                  stream=torch.cuda.current_stream(dev()))
        assert name == kernel, f"pick_kernel chose {name}"
        return [y]
    old = nt.engine.set_variants(*c["flags"])
    try:
        SO.run_behind_blocker(case_of(f"clasfv_run_conv[{TL.case_id(c)}]", call, inputs, [y]))
    finally:
        nt.engine.set_variants(*old)


@gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_run_decoder_behind_a_blocked_stream(dtype):
    from oracle import layer_ref as LR
    from tests import test_layers_gpu as TL
    nt = TL.net(dtype, "float")
    n, t, h, w = nthw = min(TL.DEC_SHAPES, key=lambda s: s[0] * s[1] * s[2] * s[3])
    taps = []
    for i, s in enumerate(LR.tap_shapes(t, h, w)):
        gens = [torch.Generator().manual_seed(1000 * k + i) for k in (1, 2)]
        a, b = (LR.to_channels_last(LR.signed_unit((n, 64) + s, g, torch.float32), 64, torch.float32).to(dev()) for g in gens)
        taps.append((torch.empty_like(a), a, b))
    seg = torch.empty(n * 2 * t * h * w, device=dev())
    mot = torch.empty(n * 4 * t * h * w, device=dev())

    def call():
        nt.engine.run_decoder([b for b, _, _ in taps], nthw, seg, mot, stream=torch.cuda.current_stream(dev()))
        return [seg, mot]
    SO.run_behind_blocker(case_of(f"clasfv_run_decoder[{dtype}-{'x'.join(map(str, nthw))}]", call, taps, [seg, mot]))


def test_launcher_cases_name_every_conv_kernel():
    from tests import test_layers_gpu as TL
    names = conv_kernel_names()
    assert {k for d, k in names if d == "fp32"} == TL.FP32_KERNELS == {c["kernel"] for c in TL.CASES if c["dtype"] == "fp32"}
    assert {k for d, k in names if d == "bf16"} == TL.BF16_KERNELS == {c["kernel"] for c in TL.CASES if c["dtype"] == "bf16"}


# ---- two streams -----------------------------------------------------------------------------------------
_PAIRS = {}
PAIR_HANDLES, PAIR_STREAMS = 4, 3   # candidates: fresh handles, each with three fresh streams and the NULL stream


def forward_pairs():
    """{"streams": (model, s1, s2), "null": (model, s1, NULL stream)}: for each, the first candidate found on
    which a forward on the second stream completes on the device while a forward on the first sits behind a
    short blocker (None if there is none), searched once per session.

    Whether two given streams can overlap at all is not the library's to decide. Measured on the MI355X, a
    given (handle, ordered stream pair) gives the same outcome every time, and most pairs do not overlap
    (profiles/stream_order_mi355x.txt, section 4); the supposed cause is that the runtime serves all streams,
    the engine's side streams included, from a few hardware queues. What the library decides is whether
    overlap is possible: a context, arena, side stream or event shared between two streams, or a device
    synchronisation, would order B behind A on every candidate. So the search goes over up to four fresh
    handles, each with three fresh streams (and the NULL stream: four contexts, what a handle keeps), and
    the test then runs its full protocol on the pair found and fails, saying so, if none was."""
    if _PAIRS:
        return _PAIRS
    from clasfv_amd.model import R2plus1D_18_MotionNet
    _PAIRS.update(streams=None, null=None)
    null, tried = torch.cuda.default_stream(dev()), {"streams": 0, "null": 0}
    for h in range(PAIR_HANDLES):
        model = R2plus1D_18_MotionNet(pretrained=False, weights="echo")
        ca, cb = (case_forward("fp32", SMALL, key=k, model=model) for k in ("A", "B"))
        ss = [torch.cuda.Stream(dev()) for _ in range(PAIR_STREAMS)]
        ca.reset(ca.real)
        for st in [null] + ss:   # the handle's four contexts and their side streams
            ca.warm(st)
        for s1 in ss:
            for kind, s2 in [("null", null)] + [("streams", s) for s in ss if s is not s1]:
                if _PAIRS[kind] is None:
                    tried[kind] += 1
                    if SO.overlaps(ca, cb, s1, s2):
                        _PAIRS[kind] = (model, s1, s2)
        if all(_PAIRS.values()):
            break
    print(f"STREAM_PAIR forward pairs: two streams found after {tried['streams']} candidates: {_PAIRS['streams'] is not None}; "
          f"stream and NULL stream found after {tried['null']} candidates: {_PAIRS['null'] is not None} ({h + 1} handles)")
    return _PAIRS


@gpu
@pytest.mark.parametrize("b_on_null", [False, True], ids=["two-side-streams", "B-on-the-NULL-stream"])
def test_forwards_on_two_streams_do_not_wait_for_each_other(b_on_null):
    """One handle, two streams (per-stream contexts, side streams and events): with forward A behind its
    stream's blocker, forward B on another stream (or on the NULL stream) returns at once, completes on the
    device and equals its serial result while A's blocker still runs; then A equals its own. Run on the
    first (handle, stream pair) of forward_pairs()' bounded search on which the runtime lets two forwards
    overlap at all; none found is a failure."""
    found = forward_pairs()["null" if b_on_null else "streams"]
    assert found is not None, (f"on none of {PAIR_HANDLES} handles x {PAIR_STREAMS} streams did a forward on "
                               f"{'the NULL stream' if b_on_null else 'a second stream'} complete while another sat behind a "
                               f"blocker: the engine orders forwards on different streams behind one another, or the "
                               f"runtime runs every candidate pair in turn")
    model, s1, s2 = found
    SO.run_two_streams(case_forward("fp32", SMALL, key="A", model=model), case_forward("fp32", SMALL, key="B", model=model),
                       s1, s2)


@gpu
def test_normalize_on_two_streams_with_two_workspaces():
    """No stream of the library's own, and two streams the runtime runs side by side: B completes on the device
    while A's blocker runs."""
    SO.run_two_streams(case_normalize("norm-A"), case_normalize("norm-B"))


# ---- the Python layer under torch.cuda.stream(S) ---------------------------------------------------------
def py_model():
    x = pair(lambda r: r.uniform(0, 1, SMALL).astype(np.float32), "py-model")
    return case_of("model(x)", lambda: list(model_of("fp32")(x[0])), [x])


def py_build_clips():
    from clasfv_amd import fuse_utils as FU
    table, _ = FU.clip_table(70, 3, 1, True)
    vid = pair(lambda r: r.standard_normal((3, 70, H, W)).astype(np.float32), "py-clips")
    return case_of("FU.build_clips", lambda: [FU.build_clips(vid[0], table, True)], [vid])


def py_pass_labels():
    from clasfv_amd import fuse_utils as FU
    table, clip0 = FU.clip_table(70, 3, 1, True)
    x = pair(lambda r: r.normal(0.0, 2.0, (len(table), 2, 32, H, W)).astype(np.float32), "py-labels")

    def call():   # pass k writes its T - k frames only: the rest of its row is what torch.empty found there
        lab = FU.pass_labels(x[0], clip0, 70, 1, True)
        return [lab[k, :70 - k] for k in range(3)]
    return case_of("FU.pass_labels", call, [x])


def py_logit_margin():
    from clasfv_amd import fuse_utils as FU
    x = pair(lambda r: r.normal(0.0, 2.0, (2, 2, 32, H, W)).astype(np.float32), "py-margin")
    return case_of("FU.logit_margin", lambda: [FU.logit_margin(x[0])], [x])


def py_fuse_votes():
    from clasfv_amd import fuse_utils as FU
    lab = pair(lambda r: (r.random((3, 12, H, W)) < 0.5).astype(np.uint8), "py-fuse")
    return case_of("FU.fuse_votes", lambda: [FU.fuse_votes(lab[0], 1, "simple")], [lab])


def _videos():
    """(buffer, A, A') of normalised (3, 40, 16, 32) synthetic echo videos: two shifted passes of one resampled
    clip each."""
    import clasfv_amd.synthetic as S
    from oracle import fuse_ref
    a = D(fuse_ref.zeroone_normalizer(S.echo_video(40, 16, 32, seed=1)))
    b = D(fuse_ref.zeroone_normalizer(S.echo_video(40, 16, 32, seed=2, period=23)))
    return torch.empty_like(a), a, b


def py_segment():
    from clasfv_amd import fuse_utils as FU
    vid = _videos()
    model = model_of("fp32")
    return case_of("FU.segment_a_video_with_fusion_device",
                   lambda: [FU.segment_a_video_with_fusion_device(vid[0], model, num_clips=2, fuse_method="simple")], [vid])


def py_sharded():
    from clasfv_amd import dist as DI
    vid = _videos()
    model = model_of("fp32")
    return case_of("dist.segment_videos_sharded",
                   lambda: [DI.segment_videos_sharded([vid[0]], model, num_clips=2, step=1, fuse_method="simple")[0]], [vid])


def py_preprocess():
    from clasfv_amd.preprocess import preprocess_video
    frames = pair(lambda r: r.integers(0, 256, (6, 20, 24, 3), dtype=np.uint8), "py-pre")
    return case_of("preprocess_video + zeroone_normalize_", lambda: [preprocess_video(frames[0], 16, 16, device=dev())],
                   [frames])


def py_warp():
    from clasfv_amd.warp import warp
    n, c, h, w = 2, 3, 9, 11
    img = pair(lambda r: r.standard_normal((n, c, h, w)).astype(np.float32), "py-warp-img")
    mot = pair(lambda r: np.tanh(r.normal(0, 0.4, (n, 2, h, w))).astype(np.float32), "py-warp-mot")
    gout = pair(lambda r: _grad_out(r, (n, c, h, w)), "py-warp-gout")
    img[0].requires_grad_()
    mot[0].requires_grad_()

    def call():
        out = warp(img[0], mot[0])
        gi, gm = torch.autograd.grad(out, [img[0], mot[0]], gout[0])   # the backward kernel, inside the stream context
        return [out.detach(), gi, gm]
    return case_of("warp + backward", call, [img, mot, gout], close={1: (GIMG_RTOL, GIMG_ATOL)})


def py_track():
    from clasfv_amd.warp import track
    n, c, h, w, t, p = 1, 2, 24, 20, 6, 3
    img = pair(lambda r: r.standard_normal((n, c, h, w)).astype(np.float32), "py-track-img")
    mot = pair(lambda r: np.tanh(r.normal(0, 0.4, (n, 4, t, h, w))).astype(np.float32), "py-track-mot")
    gout = pair(lambda r: _grad_out(r, (p, n, c, h, w)), "py-track-gout")
    img[0].requires_grad_()
    mot[0].requires_grad_()

    def call():
        out = track(img[0], mot[0], 0, p)
        gi, gm = torch.autograd.grad(out, [img[0], mot[0]], gout[0])   # p clasfv_warp_backward calls and torch's own ops
        return [out.detach(), gi, gm]
    return case_of("track + backward", call, [img, mot, gout], close={1: (CHAIN_RTOL, CHAIN_ATOL), 2: (CHAIN_RTOL, CHAIN_ATOL)})


def py_lv_curve():
    from clasfv_amd.echo import lv_curve
    masks = pair(lambda r: _ellipses(r, 5, 31, 17), "py-lv")

    def call():
        c = lv_curve(masks[0])
        return [c.area, c.geom]
    return case_of("echo.lv_curve", call, [masks])


PYTHON_CASES = {"model": py_model, "build_clips": py_build_clips, "pass_labels": py_pass_labels,
                "logit_margin": py_logit_margin, "fuse_votes": py_fuse_votes, "segment_a_video": py_segment,
                "segment_videos_sharded": py_sharded, "preprocess_video": py_preprocess, "warp_backward": py_warp,
                "track_backward": py_track, "lv_curve": py_lv_curve}


@gpu
@pytest.mark.parametrize("which", list(PYTHON_CASES))
def test_python_layer_under_a_blocked_stream(which):
    """The package's wrappers take the current stream of the tensors' device: under torch.cuda.stream(S) every
    kernel, torch's own ops between them and the autograd backward land on S, and no wrapper waits for the
    device (the warm-up has paid the one pageable upload of a clip table; it is cached afterwards)."""
    SO.run_behind_blocker(PYTHON_CASES[which]())


@gpu
def test_video_stream_results_under_a_blocked_stream():
    """VideoStream.run under torch.cuda.stream(S) with S blocked: the masks of the serial run. Results only:
    run() uploads from the host on its own copy stream and waits once per call for its masks, as documented (so
    it returns after the blocker has ended, which is asserted, as is that it was called while the blocker ran)."""
    from clasfv_amd.stream import VideoStream
    import clasfv_amd.synthetic as S
    videos = [S.echo_video_uint8(40, 20, 24, seed=i, period=20 + 7 * i) for i in range(3)]
    vs = VideoStream(model_of("fp32"), num_clips=2, height=16, width=32)
    ref = vs.run(videos)
    SO.sync()
    s = SO.side_streams()[0]
    try:
        with torch.cuda.stream(s):
            blocker = SO.Blocker(s, SO.MIN_BLOCK)
            issued_behind = blocker.running()
            got = vs.run(videos)
            waited = not blocker.running()
    finally:   # nothing stays queued behind the blocker, whatever run() raised
        SO.sync()
    print(f"STREAM_CASE VideoStream.run blocker_s={SO.MIN_BLOCK:.3f} blocker_measured_s={blocker.measured():.3f} "
          f"issued_behind_blocker={issued_behind} returned_after_blocker_end={waited}")
    assert issued_behind, "the blocker had ended before run() was called: the case tells nothing"
    assert waited, "run() returned host masks while the stream it computes on was still blocked"
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g, r)


# ---- the clip-table cache ---------------------------------------------------------------------------------
@gpu
def test_cached_clip_table_survives_eviction_while_a_blocked_stream_reads_it():
    """fuse_utils caches device clip tables and evicts all of them past 256. A table handed to a kernel on
    stream S must not be given to another allocation while that kernel has not run: with S blocked behind
    build_clips(video, table_X), 1024 other tables requested on the default stream (as build_clips requests
    them) empty the cache three times and allocate as many new ones (all valid for T = 96, so a stale read
    stays in range). The clips on S are those of table_X. On the code before record_stream this fails on the
    MI355X: the allocator hands table_X's block to one of the new tables (profiles/stream_order_mi355x.txt)."""
    from clasfv_amd import fuse_utils as FU
    t = 96
    table_x = [(7, 40)]
    others = [[(shift, first)] for shift in range(32) for first in range(32)]   # table_X is none of them
    assert all(shift + first + 32 <= t for (shift, first), in others + [table_x])
    video = D(rng_for("cache").standard_normal((3, t, H, W)).astype(np.float32))
    FU._TABLES.clear()
    want = FU.build_clips(video, table_x, interpolate_last=False).clone()   # caches table_X, on the default stream
    other = FU.build_clips(video, others[0], interpolate_last=False)
    SO.sync()
    assert torch.equal(want[0], video[:, 7 + 40:7 + 40 + 32]) and not torch.equal(want, other)
    FU._TABLES.pop(next(k for k in FU._TABLES if k[1] == tuple(others[0])))
    s = SO.side_streams()[0]
    assert SO.default_stream_is_concurrent(), ("the default stream ran no kernel beside any of eight blocked streams: "
                                               "the runtime serialises them, and the test can show nothing")
    with torch.cuda.stream(s):   # warm: the stream's first launch
        FU.build_clips(video, table_x, interpolate_last=False)
    SO.sync()
    assert len(FU._TABLES) == 1
    with torch.cuda.stream(s):
        blocker = SO.Blocker(s, SO.MAX_BLOCK)
        got = FU.build_clips(video, table_x, interpolate_last=False)
    t0 = time.perf_counter()
    for tab in others:   # what build_clips does first: the table's device copy, from the cache or uploaded
        FU._device_table(tab, video.device)
    torch.cuda.current_stream(dev()).synchronize()
    running, t_requests = blocker.running(), time.perf_counter() - t0
    SO.sync()
    print(f"STREAM_CASE clip-table cache tables={len(others)} requests_s={t_requests:.3f} blocker_s={SO.MAX_BLOCK:.3f} "
          f"blocker_measured_s={blocker.measured():.3f} evictions_done_before_blocker_end={running}")
    assert running, "the blocker ended before the other tables were requested: the test tells nothing"
    assert torch.equal(got, want), "the clips built behind the blocker are not those of table_X"
