"""Two host restatements of the mask cleanup rule (include/clasfv.h, clasfv_fuse_votes with CLASFV_FUSE_CLEAN).

``clean_scipy`` follows cleanupBinary of the reference (src/utils/camus_validate.py:284-352) with scipy.ndimage
in place of scikit-image, which this project does not have: ``label`` with a 3 x 3 structure, the filled area by
``binary_fill_holes`` with that structure on each region's bounding box, ``label`` of the complement with the
default (4-connected) structure and ``bincount < holesize``; ties go to the first region in label order.
``clean_flood`` is written from the five steps of the rule's text with plain flood fills and nothing else.
The two agree frame for frame (tests/test_cleanup_host.py); the GPU tests compare the kernel's bytes with them.
"""
import numpy as np
from scipy import ndimage as ndi

N8 = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
N4 = [(-1, 0), (0, -1), (0, 1), (1, 0)]


def clean_scipy(frame, holesize=128):
    """One (H,W) frame -> (cleaned uint8 frame, kept component's filled area or 0, pixels filled by step 4)."""
    frame = np.asarray(frame)
    member = frame == 1
    if not member.any():
        return frame.astype(np.uint8), 0, 0
    ones = np.ones((3, 3), bool)
    lab, n = ndi.label(member, structure=ones)
    best, best_area = 0, -1
    for k, sl in enumerate(ndi.find_objects(lab), start=1):  # labels ascend with the first pixel in row-major order
        if (sl[0].stop - sl[0].start) * (sl[1].stop - sl[1].start) <= best_area:
            continue  # a filled area is at most its box, and a later equal one loses the tie
        area = int(ndi.binary_fill_holes(lab[sl] == k, structure=ones).sum())
        if area > best_area:
            best, best_area = k, area
    kept = lab == best
    rest, _ = ndi.label(~kept)
    small = np.bincount(rest.ravel()) < holesize
    small[0] = False
    filled = small[rest]
    out = np.where(kept | filled, 1, np.where(member, 0, frame)).astype(np.uint8)
    return out, best_area, int(filled.sum())


def _components(pred, nbrs):
    """[(sorted pixel list)] of the components of a boolean map, in order of their first pixel."""
    h, w = pred.shape
    seen = np.zeros((h, w), bool)
    comps = []
    for i in range(h):
        for j in range(w):
            if not pred[i, j] or seen[i, j]:
                continue
            seen[i, j] = True
            stack, comp = [(i, j)], []
            while stack:
                a, b = stack.pop()
                comp.append((a, b))
                for da, db in nbrs:
                    c, d = a + da, b + db
                    if 0 <= c < h and 0 <= d < w and pred[c, d] and not seen[c, d]:
                        seen[c, d] = True
                        stack.append((c, d))
            comps.append(comp)
    return comps


def clean_flood(frame, holesize=128):
    """The same triple as clean_scipy, from the rule's steps 1-5."""
    frame = np.asarray(frame)
    h, w = frame.shape
    member = frame == 1
    if not member.any():                                      # 1
        return frame.astype(np.uint8), 0, 0
    best, best_area = None, -1
    for comp in _components(member, N8):                      # 1: in order of the first pixel
        region = np.zeros((h + 2, w + 2), bool)               # 2: the frame in a ring of non-members
        for a, b in comp:
            region[a + 1, b + 1] = True
        outside = next(c for c in _components(~region, N8) if (0, 0) in c)
        area = h * w - (len(outside) - (2 * (h + 2) + 2 * w))
        if area > best_area:                                  # 3: strictly greater, so the first of equals stays
            best, best_area = region[1:-1, 1:-1], area
    filled = np.zeros((h, w), bool)
    for comp in _components(~best, N4):                       # 4
        if len(comp) < holesize:
            for a, b in comp:
                filled[a, b] = True
    out = frame.astype(np.uint8).copy()                       # 5
    out[member] = 0
    out[best | filled] = 1
    return out, best_area, int(filled.sum())


def clean_video(frames, holesize=128, fn=clean_scipy):
    frames = np.asarray(frames)
    return np.stack([fn(f, holesize)[0] for f in frames.reshape((-1,) + frames.shape[-2:])]).reshape(frames.shape)


def seeded_frames(count=400, seed=0):
    """The seeded set both restatements are held to: sides 1..23, densities 0.2-0.8, some pixels set to 2,
    holesize in {1, 2, 5, 128}. Yields (frame, holesize)."""
    r = np.random.default_rng(seed)
    for n in range(count):
        h, w = int(r.integers(1, 24)), int(r.integers(1, 24))
        f = (r.random((h, w)) < r.uniform(0.2, 0.8)).astype(np.uint8)
        if n % 3 == 0:
            f[(r.random((h, w)) < 0.1) & (f == 0)] = 2
        yield f, (1, 2, 5, 128)[n % 4]


def spiral(h, w):
    """A one-pixel-wide spiral of ones wound inwards from the top left corner, one-pixel gaps between its arms:
    the walk goes on while the next pixel is free and the one after it is free or outside, else turns right,
    and ends when it can go nowhere."""
    f = np.zeros((h, w), np.uint8)
    i = j = d = 0
    f[0, 0] = 1
    blocked = 0
    while blocked < 2:
        di, dj = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        a, b, c, e = i + di, j + dj, i + 2 * di, j + 2 * dj
        if 0 <= a < h and 0 <= b < w and not f[a, b] and not (0 <= c < h and 0 <= e < w and f[c, e]):
            i, j, blocked = a, b, 0
            f[i, j] = 1
        else:
            d, blocked = (d + 1) % 4, blocked + 1
    return f
