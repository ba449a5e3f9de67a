"""clasfv_amd.beats on the GPU against tests/beats_oracle.py: the chains of every beat on injected motion, bit
for bit; track_beats end to end with the engine (synthetic weights); the skips; the whole call under the pointer
audit of tests/abi_audit.py; and the CLI's ``-c tracking`` / ``-c tracking_gif``.

Frames are 32x32 and 48x32 (the non-square one catches an x / y swap); masks are the pulsing ellipse of the
oracle, T = 100 and period 40: beats (0, 20) and (40, 60), windows from frames 0 and 35 (checked without a GPU in
tests/test_beats_host.py). The oracle's chains are computed once per frame size and shared.

Exact comparisons throughout. Tracked masks: clasfv_track is pinned bit-exact to the oracle's grid_sample loop.
Dice: the counts are integers, and one float64 addition and one division are correctly rounded on both sides.
EF: a float64 subtraction, division and multiplication of the same operands, issued as separate operations.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import abi_audit as A
from tests import beats_oracle as O
from tests.conftest import REPO

pytestmark = pytest.mark.gpu

T = 100
SIZES = [(32, 32), (48, 32)]
PAIRS, STARTS = [(0, 20), (40, 60)], [0, 35]
_CACHE = {}


def dev():
    return torch.device("cuda", 0)


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    """Equal float64 arrays bit for bit; a NaN equals a NaN (its sign and payload are not part of any result)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or not a.dtype == b.dtype == np.float64:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan])


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def masks_of(h, w):
    return cached(("masks", h, w), lambda: O.ellipse_masks(T, h, w))


@pytest.fixture(scope="module")
def model():
    from clasfv_amd.model import R2plus1D_18_MotionNet
    return R2plus1D_18_MotionNet(pretrained=False)


def video_of(h, w):
    """(3,T,h,w) float32 in [0, 1] on the device: seeded noise darkened inside the ellipse."""
    def make():
        v = np.random.default_rng(h * 100 + w).uniform(0, 1, (3, T, h, w)).astype(np.float32)
        v[:, masks_of(h, w) == 1] *= 0.25
        return v
    return D(cached(("video", h, w), make))


def check_measurements(bt, masks, chains, spacing=(1.0, 1.0)):
    """Every per-beat field of a BeatTracking against the oracle: ``chains`` {pair index: (forward, backward)}."""
    from clasfv_amd import echo
    vol = host(echo.lv_curve(D(masks), 1, spacing).volume)
    seg = masks == 1
    for i, (ed, es) in enumerate(bt.pairs):
        assert same_bits(host(bt.ef_seg[i:i + 1]), np.array([O.ef(vol[ed], vol[es])])), i
        if i not in chains:
            assert bt.starts[i] is None and bt.forward[i] is None and bt.dice_backward[i] is None
            assert np.isnan(host(bt.ef_forward)[i]) and np.isnan(host(bt.ef_backward)[i])
            continue
        fwd, bwd = chains[i]
        n = es - ed
        print(f"beat {i} ({ed}, {es}): tracked areas forward {O.area(fwd).tolist()} backward {O.area(bwd).tolist()}")
        assert bt.forward[i].dtype == torch.uint8 and bt.forward[i].is_cuda and tuple(bt.forward[i].shape) == (n,) + masks.shape[1:]
        assert np.array_equal(host(bt.forward[i]), fwd), f"beat {i}: forward chain"
        assert np.array_equal(host(bt.backward[i]), bwd), f"beat {i}: backward chain"
        assert same_bits(host(bt.dice_forward[i]), O.dice(fwd, seg[ed + 1:es + 1])), i
        assert same_bits(host(bt.dice_backward[i]), O.dice(bwd, seg[ed:es])), i
        for got, stack in ((bt.curve_forward[i], fwd), (bt.curve_backward[i], bwd)):
            ref = echo.lv_curve(D(stack), 1, spacing).cpu()
            got = got.cpu()
            assert np.array_equal(got.area, ref.area) and np.array_equal(got.area, O.area(stack))
            assert same_bits(got.geom, ref.geom), f"beat {i}: curve of the tracked masks"
        v_fwd, v_bwd = host(bt.curve_forward[i].volume), host(bt.curve_backward[i].volume)
        assert same_bits(host(bt.ef_forward[i:i + 1]), np.array([O.ef(vol[ed], v_fwd[-1])])), i
        assert same_bits(host(bt.ef_backward[i:i + 1]), np.array([O.ef(v_bwd[0], vol[es])])), i


@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
def test_track_chains_on_injected_motion(h, w):
    """Five beats that cover every place of a beat in its window (a = 0, ED in mid-window, e = 31, L = 2,
    L = 32) on smooth 3-pixel motion: every mask of every chain equals the oracle's. First, on the CPU: the
    oracle's chains with the channel pairs swapped, and with every frame index off by one, differ from the right
    ones in every frame, so a kernel call that made either mistake could not pass."""
    from clasfv_amd.beats import track_chains
    masks = masks_of(h, w)
    motion = O.smooth_motion(len(O.CASES), h, w, seed=7)
    pairs, starts = [(ed, es) for ed, es, _ in O.CASES], [s for _, _, s in O.CASES]
    right = []
    for b, (ed, es, start) in enumerate(O.CASES):
        right.append(O.beat_chains(masks, motion[b], ed, es, start))
        for wrong in (O.beat_chains(masks, motion[b], ed, es, start, swap=True),
                      O.beat_chains(masks, motion[b], ed, es, start, off=1)):
            for got, bad in zip(right[-1], wrong):
                differ = (got != bad).reshape(len(got), -1).sum(1)
                assert got.any(axis=(1, 2)).all() and differ.min() > 0, (b, differ)
    forward, backward = track_chains(D(masks), motion.to(dev()), pairs, starts)
    assert len(forward) == len(backward) == len(O.CASES)
    for b, (ed, es, _) in enumerate(O.CASES):
        for name, got, want in (("forward", forward[b], right[b][0]), ("backward", backward[b], right[b][1])):
            assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (es - ed, h, w)
            assert np.array_equal(host(got), want), f"beat {b} {name}"
    # int64 masks with another label among other values: compared with the label on the device
    wide = masks.astype(np.int64) * 3 + 2
    f3, b3 = track_chains(D(wide), motion[:2].to(dev()), pairs[:2], starts[:2], label=5)
    assert all(torch.equal(x, y) for x, y in zip(f3 + b3, forward[:2] + backward[:2]))


@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
def test_track_beats_end_to_end(h, w, model, monkeypatch):
    """track_beats with the engine: the windows, the motion it tracked through (the model's, bit for bit), every
    field against the oracle run on that motion, pairs=None, and one beat alone against the batch."""
    from clasfv_amd import beats, echo
    masks, video = masks_of(h, w), video_of(h, w)
    dmasks = D(masks)
    seen = []
    real = beats.track_chains
    monkeypatch.setattr(beats, "track_chains", lambda *a, **kw: (seen.append(a), real(*a, **kw))[1])
    bt = beats.track_beats(video, dmasks, model, pairs=PAIRS)
    assert bt.pairs == PAIRS and bt.starts == STARTS and bt.skipped == []
    (m_arg, motion, p_arg, s_arg, lab), = seen
    assert m_arg is dmasks and p_arg == PAIRS and s_arg == STARTS and lab == 1
    assert motion.dtype == torch.float32 and tuple(motion.shape) == (2, 4, 32, h, w)
    clips = beats.beat_clips(video, STARTS)
    assert torch.equal(clips, torch.stack([video[:, s:s + 32] for s in STARTS]))   # never resampled in time
    assert torch.equal(motion, model(clips)[1]), "the motion tracked through is not the model's"
    fwd, bwd = real(dmasks, motion, PAIRS, STARTS)
    assert all(torch.equal(a, b) for a, b in zip(bt.forward + bt.backward, fwd + bwd))
    field = motion.cpu()
    chains = {i: O.beat_chains(masks, field[i], ed, es, s) for i, ((ed, es), s) in enumerate(zip(PAIRS, STARTS))}
    check_measurements(bt, masks, chains)
    curve = echo.lv_curve(dmasks)
    efs, pairs = echo.ef_from_curve(curve.area, curve.volume, "test", return_edes=True)
    assert [(int(d), int(s)) for d, s in pairs] == PAIRS and len(efs) == 2
    assert same_bits(host(bt.ef_seg), np.array(efs, np.float64))
    # pairs=None: the same beats, found from the masks' area curve
    found = beats.track_beats(video, dmasks, model)
    assert found.pairs == PAIRS and found.starts == STARTS
    assert all(torch.equal(a, b) for a, b in zip(found.forward + found.backward, bt.forward + bt.backward))
    # batch independence: the second beat alone
    alone = beats.track_beats(video, dmasks, model, pairs=PAIRS[1:])
    assert alone.starts == STARTS[1:]
    for name in beats.BeatTracking.LISTS:
        a, b = getattr(alone, name)[0], getattr(bt, name)[1]
        if name.startswith("curve"):
            assert torch.equal(a.area, b.area) and same_bits(host(a.geom), host(b.geom)), name
        else:
            assert a.dtype == b.dtype and np.array_equal(host(a), host(b)), name
    for name in beats.BeatTracking.VECTORS:
        assert same_bits(host(getattr(alone, name)), host(getattr(bt, name))[1:]), name
    # the host copy and the tracked video
    d = bt.asdict()
    assert sorted(d) == sorted(beats.BeatTracking.KEYS) and np.array_equal(d["forward"][1], chains[1][0])
    tv = bt.tracked_video()
    want = masks.copy()
    for (ed, es), (f, _) in zip(PAIRS, chains.values()):
        want[ed + 1:es + 1] = f
    assert tv.dtype == torch.uint8 and np.array_equal(host(tv), want) and np.array_equal(host(dmasks), masks)


def test_skips(model, monkeypatch):
    """A beat of 33 frames is skipped beside a tracked one; masks of fewer than 32 frames skip every beat without
    a forward; a beat whose ES is the video's last frame is tracked in the last 32 frames."""
    from clasfv_amd import beats, fuse_utils
    h, w = 32, 32
    masks, video = masks_of(h, w), video_of(h, w)
    seen = []
    real = beats.track_chains
    monkeypatch.setattr(beats, "track_chains", lambda *a, **kw: (seen.append(a), real(*a, **kw))[1])
    pairs = [(10, 42), (80, 99)]
    bt = beats.track_beats(video, D(masks), model, pairs=pairs)
    assert bt.pairs == pairs and bt.starts == [None, 68] and bt.skipped == [(0, "beat longer than a clip")]
    motion = seen[0][1]
    assert tuple(motion.shape) == (1, 4, 32, h, w) and seen[0][2] == [(80, 99)] and seen[0][3] == [68]
    assert torch.equal(motion, model(torch.stack([video[:, 68:100]]))[1])
    check_measurements(bt, masks, {1: O.beat_chains(masks, motion.cpu()[0], 80, 99, 68)})
    # T' = 31 < 32 (the video keeps its 100 frames): nothing is tracked and the model is not run
    monkeypatch.setattr(fuse_utils, "run_model", lambda *a, **kw: pytest.fail("a forward for no tracked beat"))
    short = beats.track_beats(video, D(masks[:31]), model, pairs=[(0, 20)])
    assert short.starts == [None] and short.skipped == [(0, "video shorter than a clip")] and short.forward == [None]
    check_measurements(short, masks[:31], {})
    none = beats.track_beats(video, D(masks), model, pairs=[])
    assert none.pairs == [] and tuple(none.ef_seg.shape) == (0,) and none.ef_seg.dtype == torch.float64
    assert np.array_equal(host(none.tracked_video()), masks)


def test_device_refusals(model):
    """Bad calls with device tensors: ValueError naming the argument (the host-tensor ones run without a GPU)."""
    from clasfv_amd import beats
    h, w = 32, 32
    masks, video = D(masks_of(h, w)), video_of(h, w)
    motion = torch.zeros((2, 4, 32, h, w), device=dev())
    for bad, name in ((lambda: beats.track_chains(masks, motion.cpu(), PAIRS, STARTS), "motion"),
                      (lambda: beats.track_chains(masks, motion.double(), PAIRS, STARTS), "motion"),
                      (lambda: beats.track_chains(masks, motion[:1], PAIRS, STARTS), "motion"),
                      (lambda: beats.track_chains(masks, motion[..., :16], PAIRS, STARTS), "motion"),
                      (lambda: beats.track_chains(masks, motion, PAIRS, STARTS[:1]), "starts"),
                      (lambda: beats.track_chains(masks, motion, PAIRS, [0, 41]), r"starts\[1\]"),
                      (lambda: beats.track_chains(masks, motion, PAIRS, [0, 28]), r"starts\[1\]"),
                      (lambda: beats.track_chains(masks, motion, [(0, 20), (80, 99)], [0, 69]), r"starts\[1\]"),
                      (lambda: beats.track_chains(masks, motion, [(0, 20), (60, 100)], STARTS), r"pairs\[1\]"),
                      (lambda: beats.track_beats(video, masks.cpu(), model, pairs=PAIRS), "masks"),
                      (lambda: beats.track_beats(video, masks.float(), model, pairs=PAIRS), "masks"),
                      (lambda: beats.track_beats(video[:, :90], masks, model, pairs=PAIRS), "masks"),
                      (lambda: beats.track_beats(video, masks[:, :16], model, pairs=PAIRS), "masks"),
                      (lambda: beats.track_beats(video[:2], masks, model, pairs=PAIRS), "video"),
                      (lambda: beats.track_beats(video, masks, model, pairs=[(20, 0)]), r"pairs\[0\]"),
                      (lambda: beats.track_beats(video, masks, model, pairs=PAIRS, spacing=(0.0, 1.0)), "spacing")):
        with pytest.raises(ValueError, match=rf"\b{name}"):
            bad()


def test_track_beats_under_the_pointer_audit(model, monkeypatch):
    """The whole of track_beats, pairs found from the masks, under tests/abi_audit.py: every pointer of every
    call inside the existing footprint rules, in live allocations, on the current stream."""
    from clasfv_amd import _lib, beats, fuse_utils as FU
    h, w = 48, 32
    aud = A.install(monkeypatch, _lib)
    monkeypatch.setattr(FU, "_TABLES", {})
    monkeypatch.setattr(model.engine, "lib", aud)
    bt = beats.track_beats(video_of(h, w), D(masks_of(h, w)), model, spacing=(0.5, 2.0))
    torch.cuda.synchronize()
    assert bt.starts == STARTS and aud.resolver == "allocator snapshot"
    assert dict(aud.calls) == {"clasfv_lv_geometry": 3, "clasfv_build_clips": 1, "clasfv_forward": 1, "clasfv_track": 4}
    assert set(aud.calls) <= set(A.FOOTPRINT)


@pytest.mark.timeout(400)
def test_cli_tracking(tmp_path):
    """``-c tracking`` adds <name>_beat_tracking.pkl and ``-c tracking_gif`` <name>_tracking.gif (.npy without
    PIL), and nothing else; every other file is byte-identical to a run without them. The pickle holds the beats
    the ED / ES files name, tracked, with one Dice per tracked frame."""
    import clasfv_amd.synthetic as S
    vid = tmp_path / "beats100.npy"
    np.save(vid, S.echo_video_uint8(100, seed=11))
    runs = {"without": "binary,binary_video", "tracking": "binary,binary_video,tracking",
            "both": "binary,binary_video,tracking,tracking_gif"}
    files, verbose = {}, {}
    for key, content in runs.items():
        out = tmp_path / key
        out.mkdir()
        r = subprocess.run([sys.executable, "motion_segment.py", "-p", str(vid), "--synthetic-weights", "1234", "-f", "1",
                            "-v", "-c", content, "-o", str(out)], capture_output=True, text=True, timeout=180, cwd=REPO)
        assert r.returncode == 0, r.stderr[-3000:]
        files[key], verbose[key] = sorted(os.listdir(out)), r.stdout
    try:
        import PIL  # noqa: F401
        movie = "beats100_tracking.gif"
    except ImportError:
        movie = "beats100_tracking.npy"
    assert files["tracking"] == sorted(files["without"] + ["beats100_beat_tracking.pkl"])
    assert files["both"] == sorted(files["tracking"] + [movie])
    for key in ("tracking", "both"):
        for f in files["without"]:
            assert (tmp_path / key / f).read_bytes() == (tmp_path / "without" / f).read_bytes(), (key, f)
    assert (tmp_path / "both" / "beats100_beat_tracking.pkl").read_bytes() == \
        (tmp_path / "tracking" / "beats100_beat_tracking.pkl").read_bytes()
    assert (tmp_path / "both" / movie).stat().st_size > 0
    d = pickle.load(open(tmp_path / "tracking" / "beats100_beat_tracking.pkl", "rb"))
    masks = pickle.load(open(tmp_path / "tracking" / "beats100_whole_video_segmentation.pkl", "rb"))
    assert sorted(d) == sorted(["pairs", "starts", "skipped", "forward", "backward", "dice_forward", "dice_backward",
                                "curve_forward", "curve_backward", "ef_seg", "ef_forward", "ef_backward"])
    named = sorted(int(f.split("_")[3]) for f in files["without"] if "_ED_Frame_" in f)
    assert len(d["pairs"]) >= 1 and sorted(ed for ed, _ in d["pairs"]) == named and d["skipped"] == []
    for i, (ed, es) in enumerate(d["pairs"]):
        n = es - ed
        assert d["forward"][i].shape == (n,) + masks.shape[1:] and d["forward"][i].dtype == np.uint8
        assert d["dice_forward"][i].shape == d["dice_backward"][i].shape == (n,)
        assert np.array_equal(d["dice_forward"][i], O.dice(d["forward"][i], masks[ed + 1:es + 1] == 1))
        assert np.array_equal(d["curve_forward"][i]["area"], O.area(d["forward"][i]))
        assert "Beat #{:d}: ED {:d} & ES {:d} EF segmented".format(i + 1, ed, es) in verbose["tracking"]
    assert d["ef_seg"].shape == d["ef_forward"].shape == d["ef_backward"].shape == (len(d["pairs"]),)
    assert "Beat #" not in verbose["without"]
