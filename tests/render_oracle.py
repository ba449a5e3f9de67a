"""numpy float64 restatement of clasfv_render_annotated's rules (include/clasfv.h): the overlay pane, the
nearest-neighbour resize, the quantisation and the curve strip, operation for operation (numpy rounds every
product and sum, as the kernel does with contraction off), so the GPU tests compare bytes exactly.
Also the seeded inputs those tests and tests/golden/make_golden_overlay.py share."""
import math

import numpy as np

LIME = np.array([50, 205, 50], np.uint8)


def overlay_inputs(T=4, H=24, W=40, seed=31):
    """Seeded inputs of tests/golden/overlay.npz (regenerated in the tests; only the reference's outputs are
    stored): a uniform-random float32 video with an all-0 and an all-1 row per channel (both ends of the clip),
    and 0 / 1 / 2 label maps for the prediction and the truth."""
    rng = np.random.Generator(np.random.PCG64(seed))
    video = rng.uniform(0, 1, (3, T, H, W)).astype(np.float32)
    video[:, :, 0] = 0.0
    video[:, :, 1] = 1.0
    seg = rng.integers(0, 3, (T, H, W)).astype(np.uint8)
    gt = rng.integers(0, 3, (T, H, W)).astype(np.uint8)
    return dict(video=video, seg=seg, gt=gt)


def gray(video):
    v = np.asarray(video, np.float32).astype(np.float64)
    return (v[0] * 0.2989 + v[1] * 0.5870) + v[2] * 0.1140


def quantise(x):
    """floor(255 * clip(x, 0, 1)), NaN -> 0."""
    with np.errstate(invalid="ignore"):
        x = np.where(x > 0.0, np.where(x < 1.0, x, 1.0), 0.0)
    return (255.0 * x).astype(np.uint8)  # 255 * x is in [0, 255]: the cast truncates


def pane_source(video, masks, label=1, truth=None):
    """(T,H,W,3) uint8: the pane at identity size."""
    g = gray(video)
    m = np.asarray(masks) == label
    if truth is None:
        fp, fn = m, np.zeros_like(m)
    else:
        t = np.asarray(truth) == label
        fp, fn = m & ~t, ~m & t
    q, lifted = quantise(g), quantise(g + 0.3)
    rg, b = np.where(fp, lifted, q), np.where(fn, lifted, q)
    return np.stack([rg, rg, b], axis=-1)


def nearest_index(dst, src):
    """Source index of every destination index: min(floor(i * (1.0 / (dst / src))), src - 1)."""
    scale = 1.0 / (float(dst) / float(src))
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * scale).astype(np.int64), src - 1)


def strip(volume, i, Hs, Wo, thickness):
    """(Hs,Wo,3) uint8: the curve strip of frame i of a video with the given per-frame volumes."""
    v = np.asarray(volume, np.float64)
    T = len(v)
    out = np.zeros((Hs, Wo, 3), np.uint8)
    fin = v[np.isfinite(v)]
    if not len(fin) or Hs == 0:
        return out
    vmin, vmax = float(fin.min()), float(fin.max())
    S = float(T + 1) / float(Wo)
    yhi = vmax + 100.0
    with np.errstate(all="ignore"):
        sy = np.float64(Hs) / np.float64(yhi - (vmin - 100.0))
        h = thickness / 2.0
        r = np.arange(Hs, dtype=np.float64)
        for x in range(Wo):
            A = float(x) * S
            B = float(x + 1) * S
            B = B if B < float(i) else float(i)
            if not A <= B:
                continue
            on = np.zeros(Hs, bool)
            for k in range(int(math.floor(A)), min(int(math.ceil(B)) - 1, i - 1) + 1):
                v0, v1 = np.float64(v[k]), np.float64(v[k + 1])
                if not (np.isfinite(v0) and np.isfinite(v1)):
                    continue
                dk = np.float64(k)
                dk1 = dk + 1.0
                dv = v1 - v0
                ta = dk if dk > A else np.float64(A)
                tb = dk1 if dk1 < B else np.float64(B)
                va, vb = v0 + (ta - dk) * dv, v0 + (tb - dk) * dv
                ya, yb = (yhi - va) * sy, (yhi - vb) * sy
                top = (ya if ya < yb else yb) - h
                bot = (ya if ya > yb else yb) + h
                on |= (r + 1.0 > top) & (r <= bot)
            out[on, x] = LIME
    return out


def render(video, masks, volume, first=0, count=None, Hp=None, Wo=None, Ht=0, Hs=0, label=1, thickness=2.0, truth=None,
           title=None):
    """(count, Hp + Ht + Hs, Wo, 3) uint8: what clasfv_render_annotated writes."""
    _, T, H, W = np.shape(video)
    Hp = H if Hp is None else Hp
    Wo = W if Wo is None else Wo
    count = T - first if count is None else count
    src = pane_source(video, masks, label, truth)
    pane = src[:, nearest_index(Hp, H)][:, :, nearest_index(Wo, W)]
    band = np.zeros((Ht, Wo, 3), np.uint8) if title is None else np.asarray(title, np.uint8).reshape(Ht, Wo, 3)
    return np.stack([np.concatenate([pane[i], band, strip(volume, i, Hs, Wo, thickness)])
                     for i in range(first, first + count)])
