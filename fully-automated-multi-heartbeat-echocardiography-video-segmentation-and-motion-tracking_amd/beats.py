"""Beat tracking: every detected heartbeat of a whole video pushed through the motion head's fields.

The network's second output, four motion channels per clip, is what the reference uses to track an ED (end-
diastole) label forward to ES (end-systole) and an ES label back to ED, but only on its 10-frame CAMUS clips
(``get_deformed_label_forback``, src/visualization_utils.py:58-80, frame indices 0..9). Here the same two loops
run for every ED / ES pair of a video of any length ("Beat tracking"):

* ``beat_window``: the 32-frame window round a beat, inside the range ``random_start_and_end``
  (src/echonet_dataset.py:11-30) drew its training windows from;
* ``track_chains``: per beat one forward and one backward nearest-mode ``warp.track`` chain (``clasfv_track``);
* ``track_beats``: windows -> ``build_clips`` -> one batched forward that keeps the motion output ->
  ``track_chains`` -> per-frame Dice against the segmentation, ``lv_curve`` of the tracked masks and the three
  ejection fractions (segmentation alone, tracked ES, tracked ED), all on the device, as a ``BeatTracking``.

Everything is issued on the current stream of the model's device. The only host synchronisation is the peak
detection of ``pairs=None`` (the area curve goes to scipy on the host); with explicit pairs there is none.
No trained weights are available offline, so nothing here says how accurate a tracked EF is.
"""
import numbers

import numpy as np
import torch

from . import _lib, echo, fuse_utils, warp

CLIP = fuse_utils.CLIP

SHORT_VIDEO = "video shorter than a clip"
LONG_BEAT = "beat longer than a clip"
PAST_THE_END = "window past the end of the video"


def beat_window(ed, es, t):
    """The 32-frame window of the beat ``(ed, es)`` in a ``t``-frame video -> ``(start, None)``, or
    ``(None, reason)`` for a beat that cannot be tracked. Host integers only.

    With L = es - ed + 1 frames in the beat: L == 32 starts at ED; L < 32 centres the beat
    (``ed - (32 - L) // 2``) and clips that start to ``[max(es - 30, 0), min(t - 32, ed)]``, the range
    random_start_and_end draws from, in which ES is never the window's last frame. When ES is the video's last
    frame that range is empty (the reference's randint raises): the window is then the last 32 frames and ES
    its last frame, the one case outside the reference's range."""
    length = es - ed + 1
    if t < CLIP:
        return None, SHORT_VIDEO
    if length > CLIP:
        return None, LONG_BEAT
    if length == CLIP:
        if ed + CLIP > t:  # unreachable for a pair inside the video: a check, not a case
            return None, PAST_THE_END
        return ed, None
    shift = CLIP - length
    hi = min(t - CLIP, ed)
    lo = min(max(es - (CLIP - 2), 0), hi)
    return min(max(ed - shift // 2, lo), hi), None


def _as_int(v, what):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise ValueError(f"{what} = {v!r}: an integer expected")
    return int(v)


def check_pairs(pairs, t):
    """[(ed, es)] as host integers; ValueError unless every pair has 0 <= ed < es < t. Host arithmetic."""
    out = []
    for i, p in enumerate(pairs):
        try:
            ed, es = p
        except (TypeError, ValueError):
            raise ValueError(f"pairs[{i}] = {p!r}: a pair of frame indices (ed, es) expected") from None
        ed, es = _as_int(ed, f"pairs[{i}][0]"), _as_int(es, f"pairs[{i}][1]")
        if not 0 <= ed < es < t:
            raise ValueError(f"pairs[{i}] = ({ed}, {es}): 0 <= ed < es < {t} (the masks' frames) expected")
        out.append((ed, es))
    return out


def _check_masks(masks, label):
    if not torch.is_tensor(masks):
        raise TypeError(f"masks must be a torch tensor on the GPU (the library reads its device pointer), not "
                        f"{type(masks).__name__}")
    if masks.is_floating_point() or masks.is_complex() or masks.dtype == torch.bool:
        raise ValueError(f"masks of an integer dtype expected, not {masks.dtype}")
    if masks.dim() != 3 or masks.numel() == 0:
        raise ValueError(f"masks (T,H,W) with at least one frame expected, got {tuple(masks.shape)}")
    if isinstance(label, bool) or not isinstance(label, numbers.Integral) or not 0 <= label <= 255:
        raise ValueError(f"label {label!r} must be an integer in [0, 255] (tracked masks are uint8)")
    if not masks.is_cuda:
        raise ValueError(f"masks must be on the GPU (the library reads their device pointer), not on {masks.device}")


def _check_chains(masks, motion, pairs, starts, label):
    _check_masks(masks, label)
    _lib.on_gpu(motion, "motion", masks.device, torch.float32)
    t, h, w = masks.shape
    pairs = check_pairs(pairs, t)
    if motion.dim() != 5 or tuple(motion.shape[1:]) != (4, CLIP, h, w) or motion.shape[0] != len(pairs):
        raise ValueError(f"motion {(len(pairs), 4, CLIP, h, w)} expected (one window per pair, the masks' frame size), "
                         f"got {tuple(motion.shape)}")
    starts = list(starts)
    if len(starts) != len(pairs):
        raise ValueError(f"starts: {len(pairs)} window starts expected (one per pair), got {len(starts)}")
    for i, ((ed, es), s) in enumerate(zip(pairs, starts)):
        s = starts[i] = _as_int(s, f"starts[{i}]")
        if not (0 <= s <= ed and es < s + CLIP <= t):
            raise ValueError(f"starts[{i}] = {s}: the window [{s}, {s} + {CLIP}) must hold the beat ({ed}, {es}) inside "
                             f"the {t} frames")
    return pairs, starts


def track_chains(masks, motion, pairs, starts, label=1):
    """The two label chains of every beat -> ``(forward, backward)``, two lists of B uint8 0/1 device tensors.

    ``masks`` (T,H,W) of an integer dtype and ``motion`` (B,4,32,H,W) float32 on one GPU; ``pairs`` the B beats
    ``(ed, es)`` and ``starts`` their window starts: motion[b, :, f] is the field at video frame starts[b] + f.
    ``forward[b]`` (es - ed, H, W): ``masks[ed] == label`` pushed through the forward fields (channels 0, 1) of
    frames ed .. es - 1, landing on video frames ed + 1 .. es. ``backward[b]``: ``masks[es] == label`` through the
    backward fields (channels 2, 3) of frames es .. ed + 1, landing on es - 1 .. ed, stored in ascending frame
    order (backward[b][0] is the mask at ED). Nearest mode, one ``warp.track`` call per chain:
    get_deformed_label_forback's two loops with the beat's own indices. ValueError before the library is touched
    for a host tensor, another dtype or shape, a pair outside the masks or a window that does not hold its beat."""
    pairs, starts = _check_chains(masks, motion, pairs, starts, label)
    forward, backward = [], []
    with torch.no_grad():
        for b, ((ed, es), start) in enumerate(zip(pairs, starts)):
            a, e = ed - start, es - start
            field = motion[b:b + 1]
            seed = (masks[ed] == label).to(torch.float32)[None, None]
            fwd = warp.track(seed, field, a, e, forward=True, mode="nearest")
            seed = (masks[es] == label).to(torch.float32)[None, None]
            bwd = warp.track(seed, field, e, a, forward=False, mode="nearest")
            forward.append(fwd[:, 0, 0].to(torch.uint8))
            backward.append(bwd[:, 0, 0].flip(0).to(torch.uint8))
    return forward, backward


def _host(v):
    """A field as the host sees it: tensors as numpy arrays, LvCurves on the host, None and lists kept."""
    if v is None:
        return None
    if isinstance(v, echo.LvCurve):
        return v.cpu()
    if torch.is_tensor(v):
        return v.cpu().numpy()
    return v


class BeatTracking:
    """What ``track_beats`` found, aligned with ``pairs`` (every list has one entry per pair, None where the beat
    was skipped; the three EF vectors hold NaN there for the tracked ones).

    ``pairs`` [(ed, es)], ``starts`` [window start or None], ``skipped`` [(pair index, reason)], ``label``;
    ``forward`` / ``backward``: (L-1,H,W) uint8 tracked masks on frames ed+1..es / ed..es-1;
    ``dice_forward`` / ``dice_backward``: float64 (L-1,), 2|A & B| / (|A| + |B| + 1e-5) of the tracked mask A and
    the segmentation B at the frame A lands on; ``curve_forward`` / ``curve_backward``: ``echo.LvCurve`` of the
    tracked stacks; ``ef_seg``, ``ef_forward``, ``ef_backward``: float64 (len(pairs),) in per cent, nothing
    dropped (NaN and negative values stay). ``masks`` are the segmentation the beats were judged against.
    ``track_beats`` returns device tensors; ``cpu()`` the same as numpy arrays."""

    LISTS = ("forward", "backward", "dice_forward", "dice_backward", "curve_forward", "curve_backward")
    VECTORS = ("ef_seg", "ef_forward", "ef_backward")
    KEYS = ("pairs", "starts", "skipped") + LISTS + VECTORS

    def __init__(self, pairs, starts, skipped, forward, backward, dice_forward, dice_backward, curve_forward,
                 curve_backward, ef_seg, ef_forward, ef_backward, masks=None, label=1):
        self.pairs, self.starts, self.skipped = list(pairs), list(starts), list(skipped)
        self.forward, self.backward = list(forward), list(backward)
        self.dice_forward, self.dice_backward = list(dice_forward), list(dice_backward)
        self.curve_forward, self.curve_backward = list(curve_forward), list(curve_backward)
        self.ef_seg, self.ef_forward, self.ef_backward = ef_seg, ef_forward, ef_backward
        self.masks, self.label = masks, label

    def cpu(self):
        if isinstance(self.ef_seg, np.ndarray):
            return self
        kw = {k: [_host(v) for v in getattr(self, k)] for k in self.LISTS}
        kw.update({k: _host(getattr(self, k)) for k in self.VECTORS})
        return BeatTracking(self.pairs, self.starts, self.skipped, masks=_host(self.masks), label=self.label, **kw)

    def asdict(self):
        """``KEYS`` -> host values (what the CLI pickles): numpy arrays, the curves as ``LvCurve.asdict()``."""
        c = self.cpu()
        d = {k: getattr(c, k) for k in self.KEYS}
        for k in ("curve_forward", "curve_backward"):
            d[k] = [None if v is None else v.asdict() for v in d[k]]
        return d

    def tracked_video(self):
        """The (T',H,W) uint8 masks with frames ed+1 .. es of every tracked beat replaced by its forward chain
        (as ``label`` where the tracked mask is set, 0 elsewhere). Later beats win where beats overlap, which
        EDESpairs rules out."""
        dev = not isinstance(self.masks, np.ndarray)
        out = self.masks.to(torch.uint8).clone() if dev else self.masks.astype(np.uint8)
        for (ed, es), fwd in zip(self.pairs, self.forward):
            if fwd is not None:
                out[ed + 1:es + 1] = fwd * self.label
        return out


def _ef(v_ed, v_es):
    return (v_ed - v_es) / v_ed * 100


def _measure(masks, pairs, starts, skipped, forward, backward, label, spacing):
    """BeatTracking from the chains of the tracked beats (``forward`` / ``backward`` hold one stack per start that
    is not None): device arithmetic only, exact integer counts, float64 quotients."""
    dev = masks.device
    curve = echo.lv_curve(masks, label, spacing)
    vol = curve.volume
    nan = torch.full((), float("nan"), device=dev, dtype=torch.float64)
    n = len(pairs)
    fields = {k: [None] * n for k in BeatTracking.LISTS}
    ef_seg = [_ef(vol[ed], vol[es]) for ed, es in pairs]
    ef_fwd, ef_bwd = [nan] * n, [nan] * n
    tracked = [i for i, s in enumerate(starts) if s is not None]
    if tracked:
        seg = masks == label
        # one stack of all tracked frames beside the segmentation's frames they land on: one count and one
        # lv_curve launch for every chain of every beat
        got = torch.cat(list(forward) + list(backward))
        want = torch.cat([seg[pairs[i][0] + 1:pairs[i][1] + 1] for i in tracked] +
                         [seg[pairs[i][0]:pairs[i][1]] for i in tracked])
        a = got != 0
        both = (a & want).sum(dim=(1, 2))
        dice = (2 * both).to(torch.float64) / ((a.sum(dim=(1, 2)) + want.sum(dim=(1, 2))).to(torch.float64) + 1e-5)
        geo = echo.lv_curve(got, 1, spacing)
        at, half = 0, sum(f.shape[0] for f in forward)
        for i, fwd, bwd in zip(tracked, forward, backward):
            ed, es = pairs[i]
            k = es - ed
            for name, stack, lo in (("forward", fwd, at), ("backward", bwd, half + at)):
                fields[name][i] = stack
                fields["dice_" + name][i] = dice[lo:lo + k]
                fields["curve_" + name][i] = echo.LvCurve(geo.area[lo:lo + k], geo.geom[lo:lo + k])
            ef_fwd[i] = _ef(vol[ed], fields["curve_forward"][i].volume[-1])
            ef_bwd[i] = _ef(fields["curve_backward"][i].volume[0], vol[es])
            at += k
    empty = torch.empty(0, device=dev, dtype=torch.float64)
    vec = lambda xs: torch.stack(xs) if xs else empty
    return BeatTracking(pairs, starts, skipped, ef_seg=vec(ef_seg), ef_forward=vec(ef_fwd), ef_backward=vec(ef_bwd),
                        masks=masks, label=label, **fields)


def beat_clips(video, starts):
    """(B,3,32,H,W) window clips of a (3,T,H,W) device video, one per start, never resampled in time."""
    return fuse_utils.build_clips(video, [(0, s) for s in starts], interpolate_last=False)


def track_beats(video, masks, model, pairs=None, label=1, batch_size=None, spacing=(1.0, 1.0)):
    """Track every heartbeat of a segmented video through the model's motion fields -> ``BeatTracking``.

    ``video``: (3,T,H,W) on the model's GPU, normalised as for segment_a_video_with_fusion_device; ``masks``: its
    fused (T',H,W) masks of an integer dtype on the same GPU (T' <= T; with T' < T, the strict reference's
    ``step > 1``, a beat is judged against T'); ``pairs``: [(ed, es)] with 0 <= ed < es < T', or None for
    ``echo.ed_es_pairs`` of the masks' area curve, the call's only host synchronisation. A beat gets the window
    of ``beat_window`` or is skipped with its reason; the windows of the tracked beats go through the model in
    one batched ``run_model`` (``batch_size`` clips per forward), whose motion output feeds ``track_chains``.
    ``spacing``: pixel spacing per image axis for the curves. ValueError for a host tensor, a wrong shape or
    dtype, two devices or a pair outside [0, T'), before the library or a stream is touched."""
    _lib.on_gpu(video, "video")
    _check_masks(masks, label)
    dev = fuse_utils._device_of(model)
    if video.device != dev:
        raise ValueError(f"video must be on the model's device {dev}, not on {video.device}")
    if masks.device != dev:
        raise ValueError(f"masks must be on the model's device {dev}, not on {masks.device}")
    if video.dim() != 4 or video.shape[0] != 3:
        raise ValueError(f"video: a (3,T,H,W) video expected, got {tuple(video.shape)}")
    t = masks.shape[0]
    if t > video.shape[1] or tuple(masks.shape[1:]) != tuple(video.shape[2:]):
        raise ValueError(f"masks (T',H,W) with T' <= {video.shape[1]} frames of {tuple(video.shape[2:])} expected (the "
                         f"video's), got {tuple(masks.shape)}")
    sy, sx = (float(s) for s in spacing)
    if not (np.isfinite(sy) and np.isfinite(sx) and sy > 0 and sx > 0):
        raise ValueError(f"spacing must be two finite positive numbers, got {spacing!r}")
    if pairs is None:
        area = echo.lv_curve(masks, label).area.cpu().numpy()
        pairs = [(int(d), int(s)) for d, s in echo.ed_es_pairs(area)]
    pairs = check_pairs(pairs, t)
    starts, skipped = [], []
    for i, (ed, es) in enumerate(pairs):
        start, why = beat_window(ed, es, t)
        starts.append(start)
        if start is None:
            skipped.append((i, why))
    tracked = [i for i, s in enumerate(starts) if s is not None]
    forward, backward = [], []
    if tracked:
        clips = beat_clips(video, [starts[i] for i in tracked])
        _, motion = fuse_utils.run_model(model, clips, batch_size, return_motion=True)  # the logits are not used
        forward, backward = track_chains(masks, motion, [pairs[i] for i in tracked], [starts[i] for i in tracked], label)
    return _measure(masks, pairs, starts, skipped, forward, backward, label, spacing)
