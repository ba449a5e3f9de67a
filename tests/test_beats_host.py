"""clasfv_amd.beats without a GPU: the window rule against the range the reference draws its training windows
from (tests/beats_oracle.py restates it), the skip reasons, what BeatTracking hands to the host, run_model's
``return_motion`` on a stand-in model, and the refusals, each raised before the library is reached."""
import numpy as np
import pytest
import torch

from tests import beats_oracle as O


class Stub:
    """Stands where the ctypes library does: touching it is the failure looked for."""

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


def test_window_rule_by_brute_force():
    """Every (t, ed, es) with 32 <= t < 80: the window holds the beat inside the video, equals the restated rule,
    lies in the reference's range whenever that range is not empty (so ES is not the window's last frame), and
    the one case outside it is ES on the video's last frame, where the window is the last 32 frames."""
    from clasfv_amd.beats import beat_window
    seen = {"tracked": 0, "long": 0, "full": 0, "last": 0}
    for t in range(32, 80):
        for ed in range(t):
            for es in range(ed + 1, t):
                start, why = beat_window(ed, es, t)
                assert (start, why) == O.window(ed, es, t), (t, ed, es)
                length = es - ed + 1
                if length > 32:
                    assert start is None and why == "beat longer than a clip"
                    seen["long"] += 1
                    continue
                assert why is None and isinstance(start, int), (t, ed, es)
                assert 0 <= start <= ed and es < start + 32 <= t, (t, ed, es, start)
                seen["tracked"] += 1
                if length == 32:
                    assert start == ed
                    seen["full"] += 1
                    continue
                legal = O.legal_starts(ed, es, t)
                if es == t - 1:
                    assert not legal and start == t - 32 and es == start + 31, (t, ed, es, start)
                    seen["last"] += 1
                else:
                    assert legal and start in legal and es + 1 < start + 32, (t, ed, es, start)
                    centred = ed - (32 - length) // 2   # the centred start, or the legal one nearest to it
                    assert abs(start - centred) == min(abs(s - centred) for s in legal)
    assert all(seen.values()), seen


def test_skip_reasons_and_their_neighbours():
    from clasfv_amd.beats import beat_window
    assert beat_window(3, 20, 31) == (None, "video shorter than a clip")
    assert beat_window(0, 30, 31) == (None, "video shorter than a clip")
    assert beat_window(3, 20, 32) == (0, None)
    assert beat_window(10, 42, 100) == (None, "beat longer than a clip")       # L = 33
    assert beat_window(10, 41, 100) == (10, None)                                # L = 32
    assert beat_window(10, 40, 100) == (10, None)                                # L = 31: shift 1, centred at ED
    assert beat_window(10, 11, 100) == (0, None)                                 # L = 2: clipped at the video's start
    assert beat_window(50, 51, 100) == (35, None)                                # L = 2, centred
    assert beat_window(80, 99, 100) == (68, None)                                # ES last: the last 32 frames
    assert beat_window(80, 98, 100) == (68, None)                                # one before: clipped to t - 32
    assert beat_window(0, 31, 32) == (0, None)
    assert beat_window(70, 101, 100)[0] is None                                  # the check: the window leaves the video


def test_the_test_videos_have_the_beats_the_gpu_tests_expect():
    """ed_es_pairs on the area of the pulsing ellipses: the 32x32 and 48x32 test masks (period 40, T = 100) and
    the north-star recipe (period 50, T = 200), with the window starts that follow."""
    import clasfv_amd.synthetic as S
    from clasfv_amd.beats import beat_window
    from clasfv_amd.echo import ed_es_pairs
    for h, w in ((32, 32), (48, 32)):
        area = O.area(O.ellipse_masks(100, h, w))
        pairs = [(int(d), int(s)) for d, s in ed_es_pairs(area)]
        assert pairs == [(0, 20), (40, 60)], (h, w, pairs)
        assert [beat_window(d, s, 100)[0] for d, s in pairs] == [0, 35]
    area = O.area(S.ellipse_masks(200))
    pairs = [(int(d), int(s)) for d, s in ed_es_pairs(area)]
    assert pairs == [(0, 25), (50, 75), (100, 125), (150, 175)]
    assert [beat_window(d, s, 200)[0] for d, s in pairs] == [0, 47, 97, 147]


def test_run_model_returns_the_motion_on_request():
    """A stand-in model on the host: the default return is the logits alone, as before; return_motion=True adds
    the motion of the same forwards, in clip order, across batches."""
    from clasfv_amd import fuse_utils as FU
    calls = []

    def model(x):
        calls.append(x.shape[0])
        n, _, t, h, w = x.shape
        mean = x.mean(dim=1, keepdim=True)
        return mean.expand(n, 2, t, h, w) * 2, mean.expand(n, 4, t, h, w).double() * 3

    clips = torch.arange(5 * 3 * 32 * 2 * 2, dtype=torch.float32).view(5, 3, 32, 2, 2)
    seg = FU.run_model(model, clips, batch_size=2)
    assert torch.is_tensor(seg) and tuple(seg.shape) == (5, 2, 32, 2, 2) and calls == [2, 2, 1]
    seg2, mot = FU.run_model(model, clips, batch_size=2, return_motion=True)
    assert torch.equal(seg, seg2) and tuple(mot.shape) == (5, 4, 32, 2, 2) and mot.dtype == torch.float32
    assert mot.is_contiguous() and torch.equal(mot, model(clips)[1].float())
    one_seg, one_mot = FU.run_model(model, clips[:1], return_motion=True)          # one batch: no cat
    assert torch.equal(one_seg, seg[:1]) and torch.equal(one_mot, mot[:1]) and one_mot.is_contiguous()


def _tracking():
    """A BeatTracking of host arrays made by hand: pair 1 of 3 skipped."""
    from clasfv_amd.beats import BeatTracking
    from clasfv_amd.echo import LvCurve
    pairs, starts, skipped = [(0, 3), (10, 50), (60, 62)], [0, None, 40], [(1, "beat longer than a clip")]
    rng = np.random.default_rng(0)
    stack = lambda k: (rng.random((k, 4, 6)) < 0.5).astype(np.uint8)
    curve = lambda k: LvCurve(np.arange(k, dtype=np.int32), rng.random((k, 12)))
    per = lambda make: [make(3), None, make(2)]
    vec = lambda: np.array([1.0, np.nan, -2.0])
    return BeatTracking(pairs, starts, skipped, per(stack), per(stack), per(lambda k: rng.random(k)),
                        per(lambda k: rng.random(k)), per(curve), per(curve), vec(), vec(), vec(),
                        masks=np.zeros((70, 4, 6), np.int64), label=1)


def test_asdict_keys_and_alignment():
    bt = _tracking()
    assert bt.cpu() is bt
    d = bt.asdict()
    assert sorted(d) == sorted(["pairs", "starts", "skipped", "forward", "backward", "dice_forward", "dice_backward",
                                "curve_forward", "curve_backward", "ef_seg", "ef_forward", "ef_backward"])
    assert d["pairs"] == bt.pairs and d["starts"] == [0, None, 40] and d["skipped"] == [(1, "beat longer than a clip")]
    for k in ("forward", "backward", "dice_forward", "dice_backward", "curve_forward", "curve_backward"):
        assert len(d[k]) == 3 and d[k][1] is None, k
    for i, n in ((0, 3), (2, 2)):
        assert d["forward"][i].shape == (n, 4, 6) and d["forward"][i].dtype == np.uint8
        assert d["dice_backward"][i].shape == (n,) and d["dice_backward"][i].dtype == np.float64
        assert sorted(d["curve_forward"][i]) == ["area", "length", "radii", "volume"]
        assert d["curve_backward"][i]["radii"].shape == (n, 10)
    for k in ("ef_seg", "ef_forward", "ef_backward"):
        assert d[k].shape == (3,) and np.isnan(d[k][1]) and d[k][2] == -2.0, k   # nothing dropped
    import pickle
    again = pickle.loads(pickle.dumps(d))
    assert sorted(again) == sorted(d) and np.array_equal(again["forward"][2], d["forward"][2])


def test_tracked_video_replaces_the_frames_after_ed():
    bt = _tracking()
    bt.masks[:] = 7
    out = bt.tracked_video()
    assert out.dtype == np.uint8 and out.shape == (70, 4, 6)
    assert np.array_equal(out[1:4], bt.forward[0]) and np.array_equal(out[61:63], bt.forward[2])
    keep = np.ones(70, bool)
    keep[1:4] = keep[61:63] = False
    assert (out[keep] == 7).all() and (bt.masks == 7).all()


H, W = 8, 8


def _args(t=100, b=2):
    return (torch.zeros((t, H, W), dtype=torch.uint8), torch.zeros((b, 4, 32, H, W)), [(0, 20), (40, 60)][:b],
            [0, 35][:b])


def test_track_chains_refuses_host_tensors_before_the_library(stub):
    from clasfv_amd.beats import track_chains
    masks, motion, pairs, starts = _args()
    with pytest.raises(ValueError, match=r"\bmasks\b.*GPU"):
        track_chains(masks, motion, pairs, starts)
    with pytest.raises(TypeError, match=r"\bmasks\b"):
        track_chains(masks.numpy(), motion, pairs, starts)
    with pytest.raises(ValueError, match=r"\bmasks\b.*integer"):
        track_chains(masks.float(), motion, pairs, starts)
    with pytest.raises(ValueError, match=r"\bmasks\b"):
        track_chains(masks[0], motion, pairs, starts)
    with pytest.raises(ValueError, match=r"\blabel\b"):
        track_chains(masks, motion, pairs, starts, label=256)


def test_track_beats_refuses_a_host_video_before_the_library(stub):
    from clasfv_amd.beats import track_beats
    masks = _args()[0]
    with pytest.raises(ValueError, match=r"\bvideo\b.*GPU"):
        track_beats(torch.zeros((3, 100, H, W)), masks, model=None, pairs=[(0, 20)])
    with pytest.raises(TypeError, match=r"\bvideo\b"):
        track_beats(np.zeros((3, 100, H, W), np.float32), masks, model=None, pairs=[(0, 20)])


@pytest.mark.parametrize("pairs,name", [([(20, 20)], "pairs[0]"), ([(0, 20), (30, 25)], "pairs[1]"),
                                        ([(0, 100)], "pairs[0]"), ([(-1, 5)], "pairs[0]"), ([(0, 20.0)], "pairs[0][1]"),
                                        ([(0, 20, 30)], "pairs[0]"), ([5], "pairs[0]"), ([(True, 3)], "pairs[0][0]")])
def test_pairs_outside_the_masks_are_refused(pairs, name):
    from clasfv_amd.beats import check_pairs
    import re
    with pytest.raises(ValueError, match=re.escape(name)):
        check_pairs(pairs, 100)
    assert check_pairs([(0, 99), (np.int64(3), np.int32(4))], 100) == [(0, 99), (3, 4)]
