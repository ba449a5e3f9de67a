"""CPU oracle for clasfv_amd.beats (tests/test_beats_host.py, tests/test_beats_gpu.py). Imports no GPU code.

Three parts, each restated from the definitions and not from beats.py:

* ``chain`` / ``beat_chains``: a label chain as a loop of ``F.grid_sample(mode="nearest", padding_mode="border",
  align_corners=False)`` over the reference's ``generate_2dmotion_field`` grids, with the beat's own frame
  indices (get_deformed_label_forback's two loops). ``clasfv_track`` is pinned bit-exact to this
  (tests/test_track_gpu.py), so tracked masks are compared bit for bit. ``swap`` and ``off`` make the two wrong
  chains a test proves it could tell from the right one: the channel pairs swapped, every frame index off by one.
  ``CASES`` are the beats of the injected-motion test: every place of a beat in its window.
* ``dice``, ``area``, ``ef``: numpy restatements of the measurements.
* ``legal_starts`` / ``window``: the window rule, from the range ``random_start_and_end`` draws from.
"""
import numpy as np
import torch
import torch.nn.functional as F

CLIP = 32


# ---- windows ---------------------------------------------------------------------------------------------------
def legal_starts(ed, es, t):
    """Every start the reference's random_start_and_end can return for a beat shorter than the clip in a video
    of at least a clip: np.random.randint(max(ed - shift + 1, 0), min(t - 32 + 1, ed + 1)) with
    shift = 32 - (es - ed + 1); an empty list where randint would raise."""
    shift = CLIP - (es - ed + 1)
    return list(range(max(ed - shift + 1, 0), min(t - CLIP + 1, ed + 1)))


def window(ed, es, t):
    """(start, None) or (None, reason): the rule of beats.beat_window, restated through ``legal_starts``."""
    length = es - ed + 1
    if t < CLIP:
        return None, "video shorter than a clip"
    if length > CLIP:
        return None, "beat longer than a clip"
    if length == CLIP:
        return (ed, None) if ed + CLIP <= t else (None, "window past the end of the video")
    legal = legal_starts(ed, es, t)
    if not legal:                       # ES is the video's last frame: the last 32 frames
        return min(t - CLIP, ed), None
    centred = ed - (CLIP - length) // 2
    return min(legal, key=lambda s: (abs(s - centred), s)), None


# ---- test material ---------------------------------------------------------------------------------------------
def lv_phase(t, period):
    return 0.5 * (1.0 + np.cos(2.0 * np.pi * np.asarray(t, np.float64) / period))


def ellipse_masks(t, h, w, period=40):
    """(t,h,w) uint8 masks of a pulsing ellipse scaled to the frame: a = h(0.20 + 0.09 phi) rows,
    b = w(0.09 + 0.045 phi) columns."""
    f = np.arange(t)[:, None, None]
    y = np.arange(h)[None, :, None]
    x = np.arange(w)[None, None, :]
    phi = lv_phase(f, period)
    a, b = h * (0.20 + 0.09 * phi), w * (0.09 + 0.045 * phi)
    return ((((y - h / 2.0) / a) ** 2 + ((x - w / 2.0) / b) ** 2) <= 1.0).astype(np.uint8)


def smooth_motion(n, h, w, seed, pixels=3.0):
    """(n,4,32,h,w) float32 fields: per channel and frame a 4x4 grid of uniform noise upsampled bilinearly, of
    amplitude ``pixels`` pixels (pixels * 2 / w in the normalised coordinates of grid_sample)."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand((n * 4 * CLIP, 1, 4, 4), generator=g) * 2 - 1
    fine = F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True)
    return (fine.view(n, 4, CLIP, h, w) * (pixels * 2.0 / w)).contiguous()


# (ed, es, start) in a 100-frame video, what the beat covers of its window [a, e] = [ed - start, es - start]
CASES = [(0, 20, 0),      # a = 0
         (40, 60, 35),    # ED in mid-window: a = 5, e = 25
         (80, 99, 68),    # ES on the video's last frame: e = 31
         (50, 51, 35),    # L = 2: one step each way
         (10, 41, 10)]    # L = 32: the whole window, a = 0 and e = 31


# ---- chains ----------------------------------------------------------------------------------------------------
def grid(motion2, h, w):
    """generate_2dmotion_field (src/transform_utils.py:14-34): (1,h,w,2) from a (1,2,h,w) field."""
    gy, gx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    return torch.stack((gx[None] + motion2[:, 0], gy[None] + motion2[:, 1]), 3)


def chain(seed, field, frames, channels):
    """[mask after each step]: ``seed`` (h,w) 0/1 pushed through field[channels, f] for f in ``frames``."""
    h, w = seed.shape
    img = torch.as_tensor(np.asarray(seed), dtype=torch.float32)[None, None]
    out = []
    for f in frames:
        img = F.grid_sample(img, grid(field[None, channels, f], h, w), mode="nearest", padding_mode="border",
                            align_corners=False)
        out.append(img[0, 0].numpy().astype(np.uint8))
    return out


def beat_chains(masks, field, ed, es, start, label=1, swap=False, off=0):
    """(forward (L-1,h,w), backward (L-1,h,w)) uint8 of one beat, backward in ascending frame order. ``field``:
    the beat's (4,32,h,w) window motion. Two deliberate mistakes: ``swap`` sends the forward chain through
    channels 2,3 and the backward chain through 0,1; ``off=1`` moves every frame index by one, to the field of
    the frame a step lands on instead of the one it leaves (forward + 1, backward - 1: both stay in the window)."""
    masks = np.asarray(masks)
    field = torch.as_tensor(field)
    a, e = ed - start, es - start
    fch, bch = ([2, 3], [0, 1]) if swap else ([0, 1], [2, 3])
    fwd = chain(masks[ed] == label, field, [f + off for f in range(a, e)], fch)
    bwd = chain(masks[es] == label, field, [f - off for f in range(e, a, -1)], bch)
    return np.stack(fwd), np.stack(bwd[::-1])


# ---- measurements ----------------------------------------------------------------------------------------------
def dice(a, b, eps=1e-5):
    """categorical_dice's formula per frame of two 0/1 stacks -> float64 (n,)."""
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return np.array([2 * int((x & y).sum()) / (int(x.sum()) + int(y.sum()) + eps) for x, y in zip(a, b)], np.float64)


def area(stack):
    """Pixel count per frame -> int64 (n,)."""
    return (np.asarray(stack) != 0).reshape(len(stack), -1).sum(1).astype(np.int64)


def ef(v_ed, v_es):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.float64(v_ed) - np.float64(v_es)) / np.float64(v_ed) * 100
