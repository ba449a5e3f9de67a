"""The clip, label, fusion, warp and preprocess kernels of csrc/plumbing.hip, each alone, against the
CPU oracle (oracle/fuse_ref.py, oracle/warp_ref.py) at the shapes where such kernels go wrong: scalar
fallbacks (H*W % 4 != 0, pointers off a 16-byte boundary), grid-stride loops that wrap, one-pixel axes,
ragged last blocks, degenerate votes.

Calls go through the ctypes ABI so that this file owns every buffer: each output and workspace lies
between two guard bands filled with a sentinel the kernel cannot produce (all-ones bits for float32,
0xA5 for labels); after the launch the guards are intact and every element that should be written is
written. The case tables state which kernels they reach; test_cases_reach_every_plumbing_kernel compares
that with the __global__ functions of plumbing.hip.

Every case prints one PLUMB_CASE line (kernel, shape, excluded share, largest grad_img deviation in units
of its tolerance); the MI355X log is profiles/r08a_plumbing_tests.txt.
"""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

from oracle import fuse_ref, warp_ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUMBING_HIP = os.path.join(REPO, "fully-automated-multi-heartbeat-echocardiography-video-segmentation-and-motion-"
                                  "tracking_amd", "csrc", "plumbing.hip")
GUARD = 4096        # elements on each side; a multiple of 16 bytes for both dtypes
LABEL_FILL = 0xA5   # labels are 0, 1 or 2
EINVAL, EBADSHAPE = -1, -2
NUL = ctypes.c_void_p(0)


# ---- buffers and launches -----------------------------------------------------------------------------
def dev():
    return torch.device("cuda", 0)


class Guarded:
    """numel elements of float32 / uint8 between two guard bands, sentinel-filled throughout. ``offset``
    shifts the payload that many elements off the (>= 256-byte) alignment of the allocation."""

    def __init__(self, numel, dtype=torch.float32, offset=0):
        assert dtype in (torch.float32, torch.uint8) and 0 <= offset < GUARD
        self.buf = torch.empty(numel + 2 * GUARD, dtype=dtype, device=dev())
        self.raw = self.buf.view(torch.int32) if dtype == torch.float32 else self.buf
        self.fill = -1 if dtype == torch.float32 else LABEL_FILL
        self.raw.fill_(self.fill)
        self.lo, self.hi = GUARD + offset, GUARD + offset + numel
        self.t = self.buf[self.lo:self.hi]
        assert self.t.data_ptr() % 16 == (offset * self.buf.element_size()) % 16

    def guards_intact(self):
        return bool((self.raw[:self.lo] == self.fill).all()) and bool((self.raw[self.hi:] == self.fill).all())

    def written(self):
        """Payload elements that no longer hold the sentinel."""
        return self.raw[self.lo:self.hi] != self.fill

    def untouched(self):
        return bool((self.raw == self.fill).all())


def misaligned(t, elements=1):
    """A dense copy of ``t`` whose first element lies ``elements`` past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    out = flat[elements:elements + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == elements * t.element_size() and out.is_contiguous()
    return out


def lib():
    from clasfv_amd import _lib
    return _lib.load()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def launch(name, *args):
    """Call one ABI entry point on the current stream and wait for it. A refusal (CLASFV_EINVAL /
    CLASFV_EBADSHAPE) is returned; a HIP error ends the whole session: nothing more is launched on a device
    that has faulted."""
    from clasfv_amd import _lib
    rc = getattr(lib(), name)(*args, _lib.stream_ptr(None, dev()))
    if rc in (EINVAL, EBADSHAPE):
        return rc
    if rc != 0:
        pytest.exit(f"{name}: HIP error ({rc}) {lib().clasfv_last_error()}, stopping the session", returncode=3)
    try:
        torch.cuda.synchronize()
    except RuntimeError as ex:
        pytest.exit(f"{name}: HIP error, stopping the session: {ex}", returncode=3)
    return rc


def int32_array(vals):
    arr = (ctypes.c_int32 * max(1, len(vals)))(*vals)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def hw_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---- build_clips --------------------------------------------------------------------------------------
# (H, W, T, K, step, interp, misalign): K shifted passes (shift = k * step), every clip of every pass.
#   5x7      H*W % 4 != 0: the scalar body            8x12     the 16-byte-vector body
#   129x129  H*W = 16641 > 64 * 256: the scalar loop wraps
#   260x256  H*W / 4 = 16640 > 64 * 256: the vector loop wraps (T = 33: one resampled clip, one plain)
#   T = 70 resamples down to 64, T = 90 up to 96 (and 88 up to 96), T = 64 / step 32 is plain;
#   interp = 0 at T = 70 cuts the passes to 64 frames; "video" / "clips": that buffer starts one float past
#   a 16-byte boundary, which must take the scalar body and give the same bits.
BUILD_CLIPS_CASES = [
    (5, 7, 70, 3, 1, 1, None), (5, 7, 90, 2, 2, 1, None), (5, 7, 64, 2, 32, 0, None), (5, 7, 70, 2, 1, 0, None),
    (8, 12, 70, 3, 1, 1, None), (8, 12, 90, 2, 2, 1, None), (8, 12, 64, 2, 32, 0, None),
    (129, 129, 70, 2, 1, 1, None), (260, 256, 33, 2, 1, 1, None),
    (8, 12, 70, 3, 1, 1, "video"), (8, 12, 90, 2, 2, 1, "clips"),
]
BUILD_CLIPS_KERNELS = {"build_clips_kernel"}


@pytest.mark.parametrize("case", BUILD_CLIPS_CASES, ids=lambda c: "-".join(map(str, c)))
def test_build_clips_vs_oracle(case):
    """clasfv_build_clips is bit-exact against fuse_ref.divide_to_consecutive_clips on video[:, shift:]
    for every pass of the table; both bodies (vector / scalar) give the same bits."""
    from clasfv_amd import fuse_utils as FU
    h, w, t, k, step, interp, mis = case
    video = rng_for("clips", *case[:6]).standard_normal((3, t, h, w)).astype(np.float32)
    table, _ = FU.clip_table(t, k, step, bool(interp))
    assert len({s for s, _ in table}) == k and max(s for s, _ in table) > 0
    ref = np.concatenate([fuse_ref.divide_to_consecutive_clips(video[:, s:], interpolate_last=bool(interp))
                          for s in range(0, k * step, step)])
    assert ref.shape[0] == len(table)
    v = torch.from_numpy(video).to(dev())
    if mis == "video":
        v = misaligned(v)
    tab = torch.tensor(np.asarray(table, np.int32).reshape(-1), device=dev())
    out = Guarded(ref.size, offset=1 if mis == "clips" else 0)
    assert launch("clasfv_build_clips", ptr(v), t, h, w, ptr(tab), len(table), interp, ptr(out.t)) == 0
    print(f"PLUMB_CASE build_clips_kernel {h}x{w} T={t} K={k} step={step} interp={interp} misaligned={mis} "
          f"clips={len(table)} excluded=0 gimg_dev=-")
    assert out.guards_intact(), "write outside clips"
    assert bool(out.written().all()), "clip voxels left unwritten"
    np.testing.assert_array_equal(out.t.cpu().numpy().reshape(ref.shape), ref)


# ---- pass_labels, pass_labels_margin, logit_margin -----------------------------------------------------
# (H, W, (T, step, K), misalign). (70,1,3): every pass resampled 64 -> T_k; (96,2,3): pass 0 plain, passes 1
# and 2 (94, 92 frames) resampled up from 96; (64,1,1): plain; (33,1,1): one clip resampled 32 -> 33, the
# cheapest case that wraps the vector loop while it resamples. "logits": the logits start one float past a
# 16-byte boundary; "labels": the label buffer starts one byte past a 4-byte boundary (both: scalar body).
TSK = [(70, 1, 3), (96, 2, 3), (64, 1, 1)]
PASS_LABELS_CASES = ([(5, 7, tsk, None) for tsk in TSK] + [(8, 12, tsk, None) for tsk in TSK] +
                     [(129, 129, (70, 1, 3), None), (260, 256, (64, 1, 1), None), (260, 256, (33, 1, 1), None),
                      (8, 12, (70, 1, 3), "logits"), (8, 12, (96, 2, 3), "logits"), (8, 12, (70, 1, 3), "labels"),
                      (8, 12, (96, 2, 3), "labels")])
PASS_LABELS_KERNELS = {"pass_labels_kernel<false>", "pass_labels_kernel<true>", "logit_margin_kernel"}
MARGIN_EPS = 1e-6      # float64 class margin below which a label is a matter of float32 rounding
MAX_EXCLUDED = 1e-3


def _planted_logits(rng, n, h, w):
    """N(0, 2) logits (n,2,32,H,W) with, at the first and last five pixels of every frame: an exact tie,
    margins of +100 and -100 (softmax saturates), and l0 = l1 = +80 / -80."""
    x = rng.normal(0.0, 2.0, (n, 2, 32, h * w)).astype(np.float32)
    hw = h * w
    tie = np.zeros(hw, bool)
    for base in (0, hw - 5):
        x[:, 1, :, base] = x[:, 0, :, base]
        x[:, 0, :, base + 1], x[:, 1, :, base + 1] = -50.0, 50.0
        x[:, 0, :, base + 2], x[:, 1, :, base + 2] = 50.0, -50.0
        x[:, :, :, base + 3] = 80.0
        x[:, :, :, base + 4] = -80.0
        tie[[base, base + 3, base + 4]] = True
    return x.reshape(n, 2, 32, h, w), tie.reshape(h, w)


def _labels_reference(logits, clip0, t, step, k):
    """Per pass: labels and float64 margins of labels_from_logits over that pass's clips."""
    out = []
    for i in range(k):
        end = clip0[i + 1] if i + 1 < k else logits.shape[0]
        out.append(fuse_ref.labels_from_logits(logits[clip0[i]:end], t - i * step, True, return_margin=True))
    return out


def _check_labels(got, ref, tie, t, step, what):
    """got (K,T,H,W) uint8 against the per-pass reference: equal wherever the float64 margin is not tiny,
    planted ties exactly 0, the tail of every row (f >= T_k) still the sentinel. Returns the excluded share
    (planted ties, which are asserted exactly, not counted)."""
    excluded = total = 0
    for i, (lab, m) in enumerate(ref):
        tk = t - i * step
        assert lab.shape[0] == tk
        g = got[i, :tk]
        assert np.all(got[i, tk:] == LABEL_FILL), f"{what}: pass {i} wrote past its {tk} frames"
        assert np.all(g != LABEL_FILL), f"{what}: pass {i} left labels unwritten"
        assert np.all(g[:, tie] == 0), f"{what}: a planted tie is not background"
        sure = np.abs(m) > MARGIN_EPS
        np.testing.assert_array_equal(g[sure], lab[sure], err_msg=f"{what}: pass {i}")
        excluded += int((~sure & ~tie[None]).sum())
        total += m.size
    return excluded / total


@pytest.mark.parametrize("case", PASS_LABELS_CASES, ids=lambda c: f"{c[0]}x{c[1]}-T{c[2][0]}s{c[2][1]}K{c[2][2]}-{c[3]}")
def test_pass_labels_vs_oracle(case):
    """clasfv_pass_labels from both logit planes against fuse_ref.labels_from_logits (softmax, temporal
    resampling, argmax in float32 as torch computes them; margin in float64): equal wherever |q1 - q0| >
    1e-6 -- well above the float32 rounding of a probability, so a differing expf cannot flip it -- with at
    most 0.1 % of the voxels excluded (the reference alone excludes none on N(0, 2) logits). The same with
    every logit's sign flipped. clasfv_logit_margin equals l1 - l0 exactly and clasfv_pass_labels_margin
    gives the two-plane labels bit for bit."""
    from clasfv_amd import fuse_utils as FU
    h, w, (t, step, k), mis = case
    table, clip0 = FU.clip_table(t, k, step, True)
    n = len(table)
    logits, tie = _planted_logits(rng_for("labels", h, w, t, step, k), n, h, w)
    cp, keep = int32_array(clip0)
    flips = (1.0, -1.0) if h * w <= 129 * 129 else (1.0,)  # the flipped run repeats the reference: small shapes
    for sign in flips:
        x = logits * np.float32(sign)
        ref = _labels_reference(x, clip0, t, step, k)
        xd = torch.from_numpy(x).to(dev())
        if mis == "logits":
            xd = misaligned(xd)
        lab = Guarded(k * t * h * w, torch.uint8, offset=1 if mis == "labels" else 0)
        assert launch("clasfv_pass_labels", ptr(xd), k, cp, t, step, h, w, 1, ptr(lab.t)) == 0
        assert lab.guards_intact(), "write outside labels"
        got = lab.t.cpu().numpy().reshape(k, t, h, w)
        share = _check_labels(got, ref, tie, t, step, f"sign {sign:+.0f}")
        print(f"PLUMB_CASE pass_labels_kernel<false> {h}x{w} T={t} step={step} K={k} misaligned={mis} sign={sign:+.0f} "
              f"excluded={share:.2e} gimg_dev=-")
        assert share <= MAX_EXCLUDED
        # the margin exchange: d = l1 - l0 exactly, and the same labels from it bit for bit
        mar = Guarded(n * 32 * h * w)
        assert launch("clasfv_logit_margin", ptr(xd), n, h, w, ptr(mar.t)) == 0
        assert mar.guards_intact() and bool(mar.written().all())
        assert torch.equal(mar.t.view(n, 32, h, w), xd[:, 1] - xd[:, 0])
        md = misaligned(mar.t) if mis == "logits" else mar.t
        lab2 = Guarded(k * t * h * w, torch.uint8, offset=1 if mis == "labels" else 0)
        assert launch("clasfv_pass_labels_margin", ptr(md), k, cp, t, step, h, w, 1, ptr(lab2.t)) == 0
        assert lab2.guards_intact(), "write outside labels (margin form)"
        assert torch.equal(lab2.t, lab.t), "margin form differs from the two-plane form"
        print(f"PLUMB_CASE pass_labels_kernel<true>+logit_margin_kernel {h}x{w} T={t} step={step} K={k} "
              f"misaligned={mis} sign={sign:+.0f} excluded=0 gimg_dev=-")
    del keep


# (n, H, W, misalign): 3 x 300x300 is 8.64 M floats > 8192 * 256 * 4, so the grid-stride loop wraps; "in" /
# "out": that pointer one float past a 16-byte boundary (the scalar fallback).
LOGIT_MARGIN_CASES = [(1, 5, 7, None), (2, 8, 12, "in"), (2, 8, 12, "out"), (2, 5, 7, "in"), (3, 300, 300, None),
                      (1, 129, 129, "in")]


@pytest.mark.parametrize("case", LOGIT_MARGIN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_logit_margin_exact(case):
    n, h, w, mis = case
    x = torch.from_numpy(rng_for("margin", n, h, w).normal(0, 2, (n, 2, 32, h, w)).astype(np.float32)).to(dev())
    if mis == "in":
        x = misaligned(x)
    out = Guarded(n * 32 * h * w, offset=1 if mis == "out" else 0)
    assert launch("clasfv_logit_margin", ptr(x), n, h, w, ptr(out.t)) == 0
    print(f"PLUMB_CASE logit_margin_kernel n={n} {h}x{w} misaligned={mis} excluded=0 gimg_dev=-")
    assert out.guards_intact(), "write outside margin"
    assert bool(out.written().all()), "margins left unwritten"
    assert torch.equal(out.t.view(n, 32, h, w), x[:, 1] - x[:, 0])


# ---- fuse_votes ----------------------------------------------------------------------------------------
METHODS = {"majority": 0, "simple": 1, "staple": 2, "itkvoting": 3}
FORCE_GENERIC = 0x100
PASS_SETS = ("noisy", "zeros", "ones", "one_hot", "split", "mixed")


def _frames_for(k, step):
    """The shortest T (plus two frames) at which an output frame sees all K votes."""
    return max(6, (k - 1) * step + 3)


# (H, W, K, step): 5x7 is below the 1024-thread block and odd; 31x33 = 1023 and 25x41 = 1025 sit on either
# side of it; K = 16 / 17 is the packed / generic SIMPLE boundary, K = 64 the generic kernel's full mask.
FUSE_SHAPES = ([(5, 7, k, 1) for k in (1, 2, 16, 17, 64)] + [(5, 7, 16, 3), (5, 7, 17, 3)] +
               [(31, 33, 2, 1), (31, 33, 17, 1), (31, 33, 64, 1), (31, 33, 16, 3), (25, 41, 2, 1), (25, 41, 16, 1), (25, 41, 17, 3),
                (40, 48, 1, 1), (40, 48, 16, 1), (40, 48, 17, 1), (40, 48, 2, 3)])
FUSE_CASES = [s + (ps,) for s in FUSE_SHAPES for ps in PASS_SETS if not (ps in ("one_hot", "split") and s[2] == 1)]
# 224x224 at K = 4: the packed kernel needs 147 KB of LDS and raises the attribute; 260x256 at K = 17: the
# generic kernel needs 65 KB and raises its own.
FUSE_BIG_CASES = [(224, 224, 4, 1, 6, "simple"), (260, 256, 17, 1, 20, "simple_generic")]


def _simple_kernel(k, hw, force_generic):
    """launch_fuse_votes' choice, restated: the packed kernel for K <= 16 while 3 * HW fits LDS."""
    return "fuse_simple_fast_kernel" if k <= 16 and 3 * hw + 4096 <= 160 * 1024 and not force_generic else \
        "fuse_simple_kernel"


def _fuse_kernels():
    out = set()
    for h, w, k, step, _ in FUSE_CASES:
        out |= {"fuse_majority_kernel", "fuse_staple_kernel", _simple_kernel(k, h * w, False),
                _simple_kernel(k, h * w, True)}
    for h, w, k, step, t, m in FUSE_BIG_CASES:
        out.add(_simple_kernel(k, h * w, m == "simple_generic"))
    return out


def _ellipse(h, w, t):
    yy, xx = np.mgrid[0:h, 0:w]
    a, b = h * (0.25 + 0.1 * np.sin(t / 5.0)), w * (0.25 + 0.08 * np.cos(t / 7.0))
    return ((yy - h / 2) / a) ** 2 + ((xx - w / 2) / b) ** 2 <= 1


def _pass_set(name, k, t, step, h, w):
    """K pass label videos (pass i has T - i*step frames; its frame f is video frame f + i*step)."""
    rng = rng_for("fuse", name, k, t, step, h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = ((yy + xx) & 1).astype(np.uint8)
    passes = []
    for i in range(k):
        n = t - i * step
        v = np.zeros((n, h, w), np.uint8)
        for f in range(n):
            tt = f + i * step
            if name == "ones" or (name == "one_hot" and i == 0):
                v[f] = 1
            elif name == "split":       # the first half of the passes vote the checkerboard, the rest its complement
                v[f] = checker if i < k // 2 else 1 - checker
            elif name == "noisy" or (name == "mixed" and (tt // 2) % 2):
                m = _ellipse(h, w, tt)
                for _ in range(int(rng.integers(0, 4))):
                    cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(1, max(2, min(h, w) // 4))
                    m ^= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
                v[f] = m
        passes.append(v)
    return passes


def _n_votes(i, k, step):
    return sum(1 for idx in range(min(i, k)) if i - idx * step >= 0)


def _labels_buffer(passes, t):
    """(K,T,H,W) uint8 with the unused tail of every row set to 0xA5: no kernel may read it (a vote other
    than 0 / 1 would change the result)."""
    k = len(passes)
    lab = np.full((k, t) + passes[0].shape[1:], LABEL_FILL, np.uint8)
    for i, p in enumerate(passes):
        lab[i, :p.shape[0]] = p
    return torch.from_numpy(lab).to(dev())


def _run_fuse(lab, k, t, step, h, w, method):
    out = Guarded((t - (step - 1)) * h * w, torch.uint8)
    assert launch("clasfv_fuse_votes", ptr(lab), k, t, step, h, w, method, ptr(out.t)) == 0
    assert out.guards_intact(), "write outside the fused video"
    assert bool(out.written().all()), "fused pixels left unwritten"
    return out.t.cpu().numpy().reshape(t - (step - 1), h, w)


@pytest.mark.parametrize("case", FUSE_CASES, ids=lambda c: f"{c[0]}x{c[1]}-K{c[2]}-s{c[3]}-{c[4]}")
def test_fuse_votes_vs_oracle(case):
    """clasfv_fuse_votes, every method, against fuse_ref.fuse_frames. Majority, ITK voting and both SIMPLE
    kernels are bit-exact. STAPLE is equal wherever the oracle's posterior has |W - 0.5| > 1e-9, with at most
    1e-4 of the pixels excluded and none on the all-background / all-foreground sets (W is 0 or 1 there).

    Frames whose vote is an exact tie by construction -- every pixel split half / half ("split" once
    2 * (K // 2) passes vote, "one_hot" at two) -- have a STAPLE posterior of 0.5 up to the last bit of a product
    (f p (1 - p) against (1 - f)(1 - q) q with f = 0.5, p = q): there the label hangs on rounding in the
    oracle itself. The test asserts that W is within 1e-9 of 0.5 on exactly those frames, compares them
    with nothing, and holds the excluded share of all other frames to the bound."""
    h, w, k, step, name = case
    t = _frames_for(k, step)
    passes = _pass_set(name, k, t, step, h, w)
    lab = _labels_buffer(passes, t)
    outs = list(range(t - (step - 1)))
    frame_of = [0] + [o + step - 1 for o in outs[1:]]
    nv = np.array([1 if o == 0 else _n_votes(i, k, step) for o, i in zip(outs, frame_of)])
    assert nv.max() == k
    for method in ("majority", "itkvoting"):
        got = _run_fuse(lab, k, t, step, h, w, METHODS[method])
        np.testing.assert_array_equal(got, fuse_ref.fuse_frames(passes, t, step, method), err_msg=method)
        print(f"PLUMB_CASE fuse_majority_kernel({method}) {h}x{w} K={k} step={step} T={t} set={name} excluded=0 gimg_dev=-")
    ref = fuse_ref.fuse_frames(passes, t, step, "simple")
    for generic in (False, True):
        got = _run_fuse(lab, k, t, step, h, w, METHODS["simple"] | (FORCE_GENERIC if generic else 0))
        np.testing.assert_array_equal(got, ref, err_msg=f"simple generic={generic}")
        print(f"PLUMB_CASE {_simple_kernel(k, h * w, generic)} {h}x{w} K={k} step={step} T={t} set={name} "
              f"excluded=0 gimg_dev=-")
    post = []
    ref = fuse_ref.fuse_frames(passes, t, step, "staple", posterior=post)
    got = _run_fuse(lab, k, t, step, h, w, METHODS["staple"])
    assert len(post) == len(ref)
    # "split": the voters are passes 0..nv-1, of which the first K // 2 vote the checkerboard
    tied = (nv == 2 * (k // 2)) if name == "split" else (nv == 2) if name == "one_hot" else np.zeros(len(nv), bool)
    excluded = total = 0
    for o, wpost in enumerate(post):
        if wpost is None:                 # one vote: copied
            np.testing.assert_array_equal(got[o], ref[o])
            continue
        if tied[o]:
            assert np.all(np.abs(wpost - 0.5) <= 1e-9)
            continue
        sure = np.abs(wpost - 0.5) > 1e-9
        np.testing.assert_array_equal(got[o][sure], ref[o][sure], err_msg=f"staple frame {o}")
        excluded += int((~sure).sum())
        total += sure.size
    share = excluded / max(total, 1)
    print(f"PLUMB_CASE fuse_staple_kernel {h}x{w} K={k} step={step} T={t} set={name} excluded={share:.2e} "
          f"tied_frames={int(tied.sum())} gimg_dev=-")
    assert share <= 1e-4
    if name in ("zeros", "ones"):
        assert excluded == 0
        assert all(p is None or np.all(p == (name == "ones")) for p in post)


@pytest.mark.parametrize("case", FUSE_BIG_CASES, ids=lambda c: f"{c[0]}x{c[1]}-K{c[2]}-T{c[4]}-{c[5]}")
def test_fuse_simple_large_frames_raise_the_lds_limit(case):
    """SIMPLE on frames whose LDS need exceeds the 64 KB default: the packed kernel at 224x224 (147 KB) and
    the generic kernel at 260x256 with 17 passes (65 KB plus its static arrays) both raise
    hipFuncAttributeMaxDynamicSharedMemorySize and equal the oracle bit for bit."""
    h, w, k, step, t, which = case
    passes = _pass_set("noisy", k, t, step, h, w)
    lab = _labels_buffer(passes, t)
    generic = which == "simple_generic"
    assert _simple_kernel(k, h * w, generic) == ("fuse_simple_kernel" if generic else "fuse_simple_fast_kernel")
    got = _run_fuse(lab, k, t, step, h, w, METHODS["simple"] | (FORCE_GENERIC if generic and k <= 16 else 0))
    print(f"PLUMB_CASE {_simple_kernel(k, h * w, generic)} {h}x{w} K={k} step={step} T={t} set=noisy excluded=0 gimg_dev=-")
    np.testing.assert_array_equal(got, fuse_ref.fuse_frames(passes, t, step, "simple"))


# ---- warp, warp_backward -------------------------------------------------------------------------------
WARP_SHAPES = [(1, 1, 1, 7), (2, 3, 9, 1), (1, 2, 1, 1), (2, 1, 5, 7), (3, 5, 24, 36), (9, 1, 484, 484)]
WARP_FLOWS = ("zero", "tanh", "centres", "border", "clipped", "strided")
WARP_KERNELS = {"warp_kernel", "warp_backward_kernel"}
GIMG_RTOL, GIMG_ATOL = 1e-5, 1e-6  # the project's bar for the atomic scatter order (tests/test_gpu.py)


# Images above this many pixels let one border pixel collect thousands of scattered terms; see
# test_warp_vs_oracle on what the data of such images look like, and why.
PILE_UP_ABOVE = 1024


def _source_coordinate(lin, flow, size):
    """The unclipped source coordinate fma(lin + flow + 1, size / 2, -0.5) in float32, as the kernel and torch
    compute it (the product of two float32 and the -0.5 are exact in float64: one rounding)."""
    g1 = ((lin + flow).astype(np.float32) + np.float32(1)).astype(np.float32)
    return (g1.astype(np.float64) * (size * 0.5) - 0.5).astype(np.float32)


def _border_axis(lin, size, low, exact):
    """Flow along one axis of ``size`` pixels that sends lin + flow to coordinate 0 (``low``) or size - 1:
    target - lin with the grid targets 1/size - 1 and 1 - 1/size. In float32 that lands within a few 1e-5
    pixels of the border, on either side: inside, the corner weights are (eps, 1 - eps) and the gradient
    multiplier is on; outside, the coordinate is clipped onto the border, the weights are exactly (0, 1) and
    the multiplier is off. ``exact``: samples that would land inside are moved half a pixel outward, so that
    every weight is 0 or 1 (see test_warp_vs_oracle on why the large shape needs that)."""
    target = np.where(low, np.float32(1.0 / size - 1.0), np.float32(1.0 - 1.0 / size)).astype(np.float32)
    flow = (target - lin).astype(np.float32)
    if exact:
        u = _source_coordinate(lin, flow, size)
        inside = np.where(low, u > 0, u < size - 1)
        flow = np.where(inside, flow + np.where(low, -1, 1) * np.float32(1.0 / size), flow).astype(np.float32)
        u = _source_coordinate(lin, flow, size)
        assert not np.where(low, u > 0, u < size - 1).any()
    return flow


def _flow(name, n, h, w, rng):
    """Host (N,2,H,W) float32 flow, or for "strided" the (N,4,3,H,W) motion whose [:, 2:, 1] slice is used."""
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "zero":
        return np.zeros((n, 2, h, w), np.float32)
    if name == "tanh":
        return np.tanh(rng.normal(0, 0.4, (n, 2, h, w))).astype(np.float32)
    if name == "centres":   # whole multiples of a pixel pitch (2/W, 2/H in grid units)
        kx, ky = rng.integers(-2, 3, (n, h, w)), rng.integers(-2, 3, (n, h, w))
        return np.stack([kx * np.float32(2.0 / w), ky * np.float32(2.0 / h)], 1).astype(np.float32)
    if name == "border":    # source at coordinate 0 or W - 1 (H - 1), in a checkerboard of which
        low = ((yy + xx) & 1).astype(bool)
        fx = _border_axis(torch.linspace(-1, 1, w).numpy()[None, :], w, low, h * w > PILE_UP_ABOVE)
        fy = _border_axis(torch.linspace(-1, 1, h).numpy()[:, None], h, ~low, h * w > PILE_UP_ABOVE)
        return np.broadcast_to(np.stack([fx, fy])[None], (n, 2, h, w)).copy()
    if name == "clipped":   # +-3 everywhere: every sample is clipped to the border
        s = np.where(((yy + xx) & 1).astype(bool), np.float32(3), np.float32(-3))
        return np.broadcast_to(np.stack([s, -s])[None], (n, 2, h, w)).astype(np.float32).copy()
    assert name == "strided"
    return np.tanh(rng.normal(0, 0.4, (n, 4, 3, h, w))).astype(np.float32)


def _ulp_diff(a, b):
    """Largest distance in float32 ulps between two finite arrays."""
    ai, bi = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, np.int64(-2 ** 31) - ai, ai)
    bi = np.where(bi < 0, np.int64(-2 ** 31) - bi, bi)
    return int(np.abs(ai - bi).max())


@pytest.mark.parametrize("flow", WARP_FLOWS)
@pytest.mark.parametrize("shape", WARP_SHAPES, ids=hw_id)
def test_warp_vs_oracle(shape, flow):
    """clasfv_warp and clasfv_warp_backward against torch's CPU grid_sample (oracle/warp_ref.py): the warped
    image and grad_motion bit for bit, grad_img within rtol 1e-5 / atol 1e-6 (float atomics scatter in
    another order than the CPU's loop). A second backward with grad_img null and a third with grad_motion
    null give the same values and leave the absent output's buffer untouched. (9,1,484,484) has more than
    8192 * 256 pixels: the grid-stride loops wrap.

    The data are chosen so that a correct kernel can meet the grad_img bar whatever order its atomics take;
    torch's own CPU sum is one ordering among many. Flows of tanh(N(0, 0.4)) reach a whole image width, so
    many samples are clipped onto the border and one border pixel of a 484x484 image collects up to 1500
    terms grad_out * weight. Reordering a float32 sum of k terms moves it by about u sqrt(k) times the size
    of its partial sums (u = 2^-24): 2e-6 of the sum itself when all terms have one sign, far under
    rtol = 1e-5, but any multiple of the bar when signed terms cancel. Measured on the MI355X with signed
    grad_out at 484x484: 0.50 to 1.15 of the bar for |grad_out| <= 1 (one element of 2.1 M over it), 0.11
    to 0.66 over 24 launches of the same data for |grad_out| <= 1/4 -- no margin, and no fault of the
    kernel. So: (a) grad_out is signed, multiples of 1/32 in [-1/4, 1/4], on images of up to 1024 pixels
    (sums of a few hundred terms at most) and non-negative, multiples of 1/32 in [0, 1/4], above (0.04
    to 0.06 of the bar over 24 launches). (b)
    Where a flow sends every sample to the border -- "clipped" always, "border" above 1024 pixels -- every
    corner weight is exactly 0 or 1, so the terms are multiples of 1/32 and their sum is exact in any
    order (58 564 terms with (eps, 1 - eps) weights measured 16 x the bar). Small "border" images keep
    the samples that land a few 1e-5 pixels inside the border (weights eps and 1 - eps, gradient
    multiplier on) next to those that are clipped onto it."""
    n, c, h, w = shape
    rng = rng_for("warp", shape, flow)
    img = rng.standard_normal((n, c, h, w)).astype(np.float32)
    gout = (rng.integers(-8 if h * w <= PILE_UP_ABOVE else 0, 9, (n, c, h, w)) / 32.0).astype(np.float32)
    mot = np.ascontiguousarray(_flow(flow, n, h, w, rng))
    mot_d = torch.from_numpy(mot).to(dev())
    if flow == "strided":
        mview = mot_d[:, 2:, 1]
        mot = mot[:, 2:, 1]
    else:
        mview = mot_d
    m_sn, m_sc = mview.stride(0), mview.stride(1)
    assert (mview.stride(2), mview.stride(3)) == (w, 1) or h * w == 1 or (h == 1 and mview.stride(3) == 1) or \
        (w == 1 and mview.stride(2) == 1)
    ri = torch.from_numpy(img).requires_grad_()
    rm = torch.from_numpy(np.ascontiguousarray(mot)).requires_grad_()
    ro = warp_ref.warp(ri, rm)
    ro.backward(torch.from_numpy(gout))
    ro, rgi, rgm = ro.detach().numpy(), ri.grad.numpy(), rm.grad.numpy()

    img_d, gout_d = torch.from_numpy(img).to(dev()), torch.from_numpy(gout).to(dev())
    out = Guarded(img.size)
    assert launch("clasfv_warp", ptr(img_d), n, c, h, w, ptr(mview), m_sn, m_sc, ptr(out.t)) == 0
    assert out.guards_intact(), "write outside the warped image"
    assert bool(out.written().all()), "warped pixels left unwritten"
    got = out.t.cpu().numpy().reshape(img.shape)

    def backward(want_gimg, want_gmot):
        gi, gm = Guarded(img.size), Guarded(n * 2 * h * w)
        if want_gimg:
            gi.t.zero_()   # accumulated atomically: the caller zeroes it
        assert launch("clasfv_warp_backward", ptr(gout_d), ptr(img_d), n, c, h, w, ptr(mview), m_sn, m_sc,
                      ptr(gi.t) if want_gimg else NUL, ptr(gm.t) if want_gmot else NUL) == 0
        assert gi.guards_intact() and gm.guards_intact(), "write outside a gradient"
        if not want_gimg:
            assert gi.untouched(), "grad_img written although null was passed"
        if not want_gmot:
            assert gm.untouched(), "grad_motion written although null was passed"
        else:
            assert bool(gm.written().all()), "grad_motion left unwritten"
        return (gi.t.cpu().numpy().reshape(img.shape) if want_gimg else None,
                gm.t.cpu().numpy().reshape(n, 2, h, w) if want_gmot else None)

    gi, gm = backward(True, True)
    _, gm_only = backward(False, True)
    gi_only, _ = backward(True, False)
    dev_gi = float((np.abs(gi - rgi) / (GIMG_ATOL + GIMG_RTOL * np.abs(rgi))).max())
    dev_gi2 = float((np.abs(gi_only - rgi) / (GIMG_ATOL + GIMG_RTOL * np.abs(rgi))).max())
    print(f"PLUMB_CASE warp_kernel+warp_backward_kernel {n}x{c}x{h}x{w} flow={flow} excluded=0 "
          f"out_ulp={_ulp_diff(got, ro)} gmot_ulp={_ulp_diff(gm, rgm)} gimg_dev={max(dev_gi, dev_gi2):.3f}")
    np.testing.assert_array_equal(got, ro)   # the one-pixel-axis shapes too: no ulp of slack was needed
    np.testing.assert_array_equal(gm, rgm)
    np.testing.assert_array_equal(gm_only, gm)
    np.testing.assert_allclose(gi, rgi, rtol=GIMG_RTOL, atol=GIMG_ATOL)
    np.testing.assert_allclose(gi_only, rgi, rtol=GIMG_RTOL, atol=GIMG_ATOL)


def test_warp_out_argument_is_checked():
    """warp(img, motion, out=) writes N*C*H*W floats through out's pointer: anything but a contiguous
    float32 tensor of img's shape on img's device is a ValueError, raised before the launch."""
    from clasfv_amd.warp import warp
    img = torch.randn(2, 3, 6, 8, device=dev())
    mot = torch.zeros(2, 2, 6, 8, device=dev())
    good = torch.full_like(img, float("nan"))
    assert warp(img, mot, out=good) is good and not bool(torch.isnan(good).any())
    bad = [torch.empty(2, 3, 6, 7, device=dev()), torch.empty(2 * 3 * 6 * 8, device=dev()),
           torch.empty(2, 3, 6, 8, device=dev(), dtype=torch.float64),
           torch.empty(2, 3, 6, 8, device=dev(), dtype=torch.float16),
           torch.empty(2, 3, 6, 16, device=dev())[..., ::2], torch.empty(2, 3, 8, 6, device=dev()).transpose(2, 3),
           torch.empty(2, 3, 6, 8)]
    for out in bad:
        with pytest.raises(ValueError):
            warp(img, mot, out=out)


# ---- preprocess_video ----------------------------------------------------------------------------------
# (T, Hs, Ws, H, W): one-pixel output axes take the scale = 0 branch; W = 129 starts a second, ragged block of
# the 128-thread rows; 3x3 -> 16x16 upsamples.
PREPROCESS_CASES = [(2, 5, 7, 1, 1), (1, 4, 4, 1, 9), (3, 9, 1, 6, 1), (2, 20, 30, 7, 129), (1, 3, 3, 16, 16)]
PREPROCESS_KERNELS = {"preprocess_video_kernel"}


@pytest.mark.parametrize("case", PREPROCESS_CASES, ids=hw_id)
def test_preprocess_video_vs_oracle(case):
    t, hs, ws, h, w = case
    frames = rng_for("pre", case).integers(0, 256, (t, hs, ws, 3), dtype=np.uint8)
    ref = fuse_ref.preprocess_frames(frames, h, w)
    out = Guarded(3 * t * h * w)
    fd = torch.from_numpy(frames).to(dev())
    assert launch("clasfv_preprocess_video", ptr(fd), t, hs, ws, h, w, ptr(out.t)) == 0
    print(f"PLUMB_CASE preprocess_video_kernel T={t} {hs}x{ws}->{h}x{w} excluded=0 gimg_dev=-")
    assert out.guards_intact(), "write outside the resized video"
    assert bool(out.written().all()), "resized pixels left unwritten"
    np.testing.assert_array_equal(out.t.cpu().numpy().reshape(ref.shape), ref)


# ---- zeroone_normalize ---------------------------------------------------------------------------------
NORMALIZE_N = [1, 63, 255, 257, 1025, 131073]
NORMALIZE_KERNELS = {"minmax_partial_kernel", "normalize_kernel"}


@pytest.mark.parametrize("n", NORMALIZE_N)
def test_zeroone_normalize_vs_oracle(n):
    """clasfv_zeroone_normalize in place on (3, n): channel 0 signed noise, channel 1 constant (the
    reference's 0/0: NaN everywhere), channel 2 signed noise with one outlier in its last element. Bit-exact
    with NaNs compared as equal; guards around the video and around a workspace of exactly
    clasfv_zeroone_workspace_bytes()."""
    rng = rng_for("norm", n)
    v = rng.standard_normal((3, n)).astype(np.float32)
    v[1] = -2.5
    v[2, -1] = 1000.0
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = fuse_ref.zeroone_normalizer(v)
    assert np.isnan(ref[1]).all() and (n == 1 or (ref[2, -1] == 1.0 and not np.isnan(ref[[0, 2]]).any()))
    wbytes = lib().clasfv_zeroone_workspace_bytes()
    assert wbytes % 4 == 0
    ws = Guarded(wbytes // 4)
    vid = Guarded(3 * n)
    vid.t.copy_(torch.from_numpy(v).reshape(-1))
    assert launch("clasfv_zeroone_normalize", ptr(vid.t), ctypes.c_int64(n), ptr(ws.t)) == 0
    print(f"PLUMB_CASE minmax_partial_kernel+normalize_kernel n={n} excluded=0 gimg_dev=-")
    assert vid.guards_intact(), "write outside the video"
    assert ws.guards_intact(), "write outside the workspace"
    got = vid.t.cpu().numpy().reshape(3, n)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(got, ref)  # NaNs at equal places compare equal


# ---- refusals ------------------------------------------------------------------------------------------
def _refused(name, args_before_out, out, code, more=()):
    rc = launch(name, *args_before_out, ptr(out.t), *more)
    assert rc == code, f"{name}: expected {code}, got {rc}"
    assert lib().clasfv_last_error()
    assert out.untouched(), f"{name} wrote its output although it refused the call"


@pytest.mark.parametrize("entry", ["clasfv_pass_labels", "clasfv_pass_labels_margin"])
def test_pass_labels_refuses_what_it_cannot_index(entry):
    """CLASFV_EINVAL before any launch, labels untouched: H or W < 1, T > 65535 (a grid dimension),
    (K - 1) * step >= T, a pass too short for one clip, and interpolate == 0 with a pass length that is no
    multiple of 32 (rounding up would read clips that were never built; rounding down leaves frames without
    logits). Buffers are as large as a launch would need."""
    planes = 1 if entry.endswith("margin") else 2

    def logits(n, h=1, w=1):
        return torch.zeros(n * planes * 32 * max(h, 1) * max(w, 1), device=dev())

    one, keep1 = int32_array([0])
    two, keep2 = int32_array([0, 2])
    three, keep3 = int32_array([0, 2, 3])
    x = logits(8, 2, 2)
    for h, w in ((0, 2), (2, 0), (-1, 2)):
        _refused(entry, (ptr(x), 1, one, 64, 1, h, w, 1), Guarded(64 * 4, torch.uint8), EINVAL)
    _refused(entry, (ptr(logits(2048)), 1, one, 65536, 1, 1, 1, 1), Guarded(65536, torch.uint8), EINVAL)
    _refused(entry, (ptr(x), 3, three, 70, 40, 2, 2, 1), Guarded(3 * 70 * 4, torch.uint8), EINVAL)   # 2 * 40 >= 70
    _refused(entry, (ptr(x), 2, two, 70, 70, 2, 2, 1), Guarded(2 * 70 * 4, torch.uint8), EINVAL)     # T_1 == 0
    _refused(entry, (ptr(x), 2, two, 40, 30, 2, 2, 1), Guarded(2 * 40 * 4, torch.uint8), EINVAL)     # T_1 = 10: no clip
    _refused(entry, (ptr(x), 2, two, 48, 32, 2, 2, 1), Guarded(2 * 48 * 4, torch.uint8), EINVAL)     # T_1 = 16: rounds to 0
    _refused(entry, (ptr(x), 1, one, 48, 1, 2, 2, 0), Guarded(48 * 4, torch.uint8), EINVAL)          # 48 -> 64 frames
    _refused(entry, (ptr(x), 2, two, 64, 1, 2, 2, 0), Guarded(2 * 64 * 4, torch.uint8), EINVAL)      # T_1 = 63 -> 64
    _refused(entry, (ptr(x), 1, one, 70, 1, 2, 2, 0), Guarded(70 * 4, torch.uint8), EINVAL)          # 70 -> 64 frames
    # the neighbours of those refusals run
    lab = Guarded(2 * 64 * 4, torch.uint8)
    assert launch(entry, ptr(x), 2, two, 64, 32, 2, 2, 0, ptr(lab.t)) == 0 and lab.guards_intact()
    lab = Guarded(2 * 48 * 4, torch.uint8)
    assert launch(entry, ptr(x), 2, two, 48, 31, 2, 2, 1, ptr(lab.t)) == 0 and lab.guards_intact()   # T_1 = 17: one clip
    del keep1, keep2, keep3


def test_fuse_votes_refuses_what_it_cannot_launch():
    """CLASFV_EINVAL for H or W < 1 and for more than 65535 output frames of majority / ITK voting (a grid
    dimension); CLASFV_EBADSHAPE for SIMPLE on frames beyond the 160 KB of LDS (404x404), from either kernel.
    The fused buffer stays untouched."""
    lab = torch.zeros(2 * 8 * 4, dtype=torch.uint8, device=dev())
    for method in METHODS.values():
        for h, w in ((0, 2), (2, 0)):
            _refused("clasfv_fuse_votes", (ptr(lab), 2, 8, 1, h, w, method), Guarded(8 * 4, torch.uint8), EINVAL)
    long = torch.zeros(65536, dtype=torch.uint8, device=dev())
    for method in (METHODS["majority"], METHODS["itkvoting"]):
        _refused("clasfv_fuse_votes", (ptr(long), 1, 65536, 1, 1, 1, method), Guarded(65536, torch.uint8), EINVAL)
    out = Guarded(65535, torch.uint8)   # the largest that runs
    assert launch("clasfv_fuse_votes", ptr(long), 1, 65535, 1, 1, 1, METHODS["majority"], ptr(out.t)) == 0
    assert out.guards_intact() and bool((out.t == 0).all())
    hw = 404 * 404
    assert hw > 160 * 1024 - 1024
    for k in (2, 17):
        big = torch.zeros(k * 3 * hw, dtype=torch.uint8, device=dev())
        for method in (METHODS["simple"], METHODS["simple"] | FORCE_GENERIC):
            _refused("clasfv_fuse_votes", (ptr(big), k, 3, 1, 404, 404, method), Guarded(3 * hw, torch.uint8), EBADSHAPE)


def test_preprocess_video_refuses_too_many_frames():
    """T is a grid dimension: T = 65536 is CLASFV_EINVAL and the output stays untouched."""
    frames = torch.zeros(65536 * 3, dtype=torch.uint8, device=dev())
    _refused("clasfv_preprocess_video", (ptr(frames), 65536, 1, 1, 1, 1), Guarded(3 * 65536), EINVAL)


# ---- coverage ------------------------------------------------------------------------------------------
def test_cases_reach_every_plumbing_kernel():
    """The kernels the case tables above claim to reach are exactly the __global__ functions of
    plumbing.hip (a template counts once per instantiation the launchers name)."""
    src = open(PLUMBING_HIP).read()
    defined = set(re.findall(r"__global__.*?void\s+(\w+)", src))
    assert len(defined) == 12, sorted(defined)
    instantiated = set(re.findall(r"hipLaunchKernelGGL\(\s*\(?([\w<>]+)\)?\s*,", src))
    claimed = (BUILD_CLIPS_KERNELS | PASS_LABELS_KERNELS | _fuse_kernels() | WARP_KERNELS | PREPROCESS_KERNELS |
               NORMALIZE_KERNELS)
    assert claimed == instantiated, (sorted(claimed ^ instantiated))
    assert {k.split("<")[0] for k in claimed} == defined
    # every table really has cases, and the tables hold the sizes that take each path
    assert any(c[0] * c[1] % 4 for c in BUILD_CLIPS_CASES) and any(c[0] * c[1] > 65536 for c in BUILD_CLIPS_CASES)
    assert any(c[0] * c[1] % 4 and c[0] * c[1] > 16384 for c in PASS_LABELS_CASES)
    assert any(c[0] * c[1] % 4 == 0 and c[0] * c[1] > 65536 for c in PASS_LABELS_CASES)
    assert any(n * 32 * h * w > 8192 * 256 * 4 for n, h, w, _ in LOGIT_MARGIN_CASES)
    assert any(n * h * w > 8192 * 256 for n, _, h, w in WARP_SHAPES)
    assert {"fuse_simple_fast_kernel", "fuse_simple_kernel"} <= _fuse_kernels()
    assert any(3 * c[0] * c[1] > 64 * 1024 for c in FUSE_BIG_CASES) and any(c[2] == 64 for c in FUSE_CASES)
