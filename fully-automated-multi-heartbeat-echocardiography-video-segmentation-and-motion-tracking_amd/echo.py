"""Ejection fraction from fused LV masks (host side: per-video 1-D / 2-D work, not data parallel).

Behaviour (not code) of the reference's EF stage, re-derived from SURVEY.md section 3.4:

* ``compute_ef_using_putative_clips(fused_segmentations, test_pat_index, return_edes=False)``
  (src/fuse_utils.py:105-148): LV area per frame -> 5/85/95th percentiles -> end-systoles are the
  area minima and end-diastoles the area maxima found by ``scipy.signal.find_peaks`` (distance 20,
  prominence half the 5-95 range), diastoles kept only when their area reaches the 85th percentile,
  frame 0 added as a diastole when the first three frames are that large -> each systole is paired
  with the latest diastole before it (``EDESpairs``, src/echonet_dataset.py:159-172) -> volumes by
  Simpson's monoplane method of disks -> EF = (EDV - ESV) / EDV * 100; negative EFs are reported and
  dropped.
* ``get2dPucks(abin, apix, npucks=10)`` (src/utils/echo_utils.py:259-385): the mask's principal axes
  (eigenvectors of the pixel-coordinate covariance, major axis first, each axis oriented so its own
  coordinate is non-negative), the mask's thick boundary (a pixel whose 4-neighbourhood, edges
  replicated, is mixed), the boundary's extent L along the major axis cut into ``npucks`` half-open
  slabs, and per slab the median distance of its boundary pixels from the major axis (NaN for an
  empty slab, as the reference); an empty mask gives (1.0, zeros), a mask whose covariance has no
  eigen-decomposition (one pixel) (0.0, zeros).
* ``compute_ef_batch``: the same for many videos on a thread pool (numpy / scipy release the GIL in
  their kernels), for the batched multi-video path.
* ``lv_curve`` / ``ef_from_curve``: the device side. ``lv_curve`` runs get2dPucks and the disk volume of EVERY
  frame of device masks in one kernel launch (clasfv_lv_geometry, csrc/lvgeom.hip) -- the per-frame volume
  curve the reference computes for each video it annotates (src/visualization_utils.py:487-493) --
  and ``ef_from_curve`` is compute_ef_using_putative_clips from such a curve (``ed_es_pairs`` is the frame
  selection both share). The host functions above stay the parity path.

Pinned by tests/golden/ef.npz, which the reference code itself produced (tests/golden/make_golden_ef.py).
"""
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from scipy.signal import find_peaks


def thick_boundary(mask):
    """Boolean map of the pixels whose 4-neighbourhood (edge pixels replicated) holds both values."""
    m = np.asarray(mask) != 0
    pad = np.pad(m, 1, mode="edge")
    stack = np.stack([pad[1:-1, 1:-1], pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]])
    return stack.any(axis=0) & ~stack.all(axis=0)


def get2dPucks(abin, apix, npucks=10):
    """(length along the major axis, npucks disk radii) of a binary mask; ``apix`` = pixel spacing
    per image axis. An empty mask gives (1.0, zeros) as in the reference."""
    mask = np.asarray(abin) > 0
    if not mask.any():
        return 1.0, np.zeros((npucks,))
    spacing = np.asarray(apix, dtype=np.float64).reshape(2, 1)
    pts = np.stack(np.nonzero(mask)) * spacing            # (2, n) pixel coordinates
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # one-pixel masks: "Degrees of freedom <= 0"
        cov = np.cov(pts, rowvar=True)
    try:  # a one-pixel mask has an undefined (NaN) covariance: (0.0, zeros) as the reference
        evals, evecs = np.linalg.eig(cov)
    except np.linalg.LinAlgError:
        return 0.0, np.zeros((npucks,))
    axes = evecs[:, np.argsort(evals)[::-1]]            # major axis first
    axes = axes * np.where(np.diag(axes) < 0, -1.0, 1.0)  # axis i points along +coordinate i
    centre = pts.mean(axis=1, keepdims=True)
    rim = np.stack(np.nonzero(thick_boundary(mask))) * spacing
    coords = np.dot((rim - centre).T, axes)             # (n_rim, 2): (along, across) the major axis
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    cuts = np.linspace(lo[0], hi[0], npucks + 1)
    slab = np.digitize(coords[:, 0], cuts, right=False) - 1  # cuts[i] <= x < cuts[i+1] -> i
    dist = np.abs(coords[:, 1])
    radii = np.array([np.median(dist[slab == i]) if np.any(slab == i) else np.nan for i in range(npucks)])
    return (hi - lo)[0], radii


def EDESpairs(diastole, systole):
    """[(ED, ES)]: every systole with the latest diastole strictly before it; a diastole already
    paired with an earlier systole is not paired again."""
    ed = np.sort(np.asarray(diastole))
    es = np.sort(np.asarray(systole))
    prev = np.searchsorted(ed, es, side="left") - 1
    pairs, last = [], -1
    for j, s in zip(prev, es):
        if j >= 0 and j != last:
            pairs.append((ed[j], s))
            last = j
    return pairs


def _disk_volume(length, radii):
    """Simpson's monoplane method: sum of npucks cylinders of height length / npucks."""
    return np.sum(np.pi * radii * radii * length / len(radii))


def ed_es_pairs(area):
    """[(ED, ES)] frame pairs of a per-frame LV area curve: the peak and percentile selection of
    compute_ef_using_putative_clips (see the module docstring)."""
    p5, p85, p95 = np.percentile(area, [5, 85, 95])
    prom = 0.50 * (p95 - p5)
    es = find_peaks(-area, distance=20, prominence=prom)[0]
    ed = [int(i) for i in find_peaks(area, distance=20, prominence=prom)[0] if area[i] >= p85]
    if np.mean(area[:3]) >= p85:
        ed.insert(0, 0)
    return EDESpairs(np.array(ed), es)


def compute_ef_using_putative_clips(fused_segmentations, test_pat_index, return_edes=False):
    seg = np.asarray(fused_segmentations)
    area = seg.sum(axis=(1, 2)).ravel()
    pairs = ed_es_pairs(area)
    frames = seg.reshape(-1, seg.shape[-2], seg.shape[-1])
    efs = []
    for d, s in pairs:
        with np.errstate(invalid="ignore", divide="ignore"):
            edv = _disk_volume(*get2dPucks((frames[d] == 1).astype(int), (1.0, 1.0)))
            esv = _disk_volume(*get2dPucks((frames[s] == 1).astype(int), (1.0, 1.0)))
            ef = (edv - esv) / edv * 100
        if ef < 0:
            print("Negative EF at patient: " + str(test_pat_index))
            continue
        efs.append(ef)
    return (efs, pairs) if return_edes else efs


def compute_ef_batch(segmentations, names=None, return_edes=False, workers=8):
    """compute_ef_using_putative_clips over many fused mask videos on a thread pool."""
    names = list(names) if names is not None else list(range(len(segmentations)))
    with ThreadPoolExecutor(max(1, workers)) as ex:
        return list(ex.map(lambda a: compute_ef_using_putative_clips(a[0], a[1], return_edes),
                           zip(segmentations, names)))


class LvCurve:
    """Per-frame LV geometry of a mask video: ``area`` (int32 pixel count), ``length`` (long axis),
    ``radii`` (..., 10) and ``volume`` (Simpson's method of disks), float64, over the leading shape of the
    masks. ``lv_curve`` returns device tensors; ``cpu()`` the same curve as numpy arrays."""

    __slots__ = ("area", "geom")

    def __init__(self, area, geom):
        self.area, self.geom = area, geom  # geom (..., 12): length, radii[10], volume, as the library writes it

    length = property(lambda self: self.geom[..., 0])
    radii = property(lambda self: self.geom[..., 1:-1])
    volume = property(lambda self: self.geom[..., -1])

    def cpu(self):
        if isinstance(self.area, np.ndarray):
            return self
        return LvCurve(self.area.cpu().numpy(), self.geom.cpu().numpy())

    def asdict(self):
        """{"area", "length", "radii", "volume"}: numpy arrays (what the CLI pickles)."""
        c = self.cpu()
        return {k: np.ascontiguousarray(getattr(c, k)) for k in ("area", "length", "radii", "volume")}


def lv_curve(masks, label=1, spacing=(1.0, 1.0)):
    """get2dPucks and the disk volume of every frame, on the device, in one kernel launch
    (clasfv_lv_geometry; include/clasfv.h states the per-frame rules). ``masks``: a device tensor (F,H,W)
    or (N,T,H,W) of an integer dtype; a pixel belongs to the structure iff it equals ``label``. uint8 masks
    are read in place, others (the int64 of warp.track_labels, of the widened masks) are compared with
    ``label`` on the device first. ``spacing`` = pixel spacing per image axis. Returns an LvCurve of device
    tensors on the masks' stream. Agrees with the host functions to float64 rounding except on frames where a
    rim pixel ties with a slab cut ("LV geometry")."""
    import torch
    from . import _lib
    if not torch.is_tensor(masks):
        raise ValueError("masks must be a tensor on the GPU (the library reads its device pointer)")
    if masks.is_floating_point() or masks.is_complex():
        raise ValueError(f"masks of an integer dtype expected, not {masks.dtype}")
    if masks.dim() not in (3, 4) or masks.numel() == 0:
        raise ValueError(f"masks (F,H,W) or (N,T,H,W) with at least one frame expected, got {tuple(masks.shape)}")
    h, w = masks.shape[-2:]
    if h * w > _lib.LV_MAX_PIXELS:
        raise ValueError(f"frames of at most {_lib.LV_MAX_PIXELS} pixels are supported, got {h} x {w}")
    sy, sx = (float(s) for s in spacing)
    if not (np.isfinite(sy) and np.isfinite(sx) and sy > 0 and sx > 0):
        raise ValueError(f"spacing must be two finite positive numbers, got {spacing!r}")
    if masks.dtype == torch.uint8 and (int(label) != label or not 0 <= label <= 255):
        raise ValueError(f"label {label!r} is not a value of uint8 masks")
    if not masks.is_cuda:
        raise ValueError(f"masks must be on the GPU (the library reads their device pointer), not on {masks.device}")
    if masks.dtype == torch.uint8:
        frames, lab = masks.contiguous(), int(label)
    else:
        # the comparison keeps a permuted input's strides; the library reads a dense (F,H,W) block
        frames, lab = (masks == label).to(torch.uint8).contiguous(), 1
    lead = tuple(masks.shape[:-2])
    area = torch.empty(lead, device=masks.device, dtype=torch.int32)
    geom = torch.empty(lead + (_lib.LV_STRIDE,), device=masks.device, dtype=torch.float64)
    lib = _lib.load()
    _lib.check(lib.clasfv_lv_geometry(_lib.ptr(frames), area.numel(), h, w, lab, sy, sx, _lib.ptr(area), _lib.ptr(geom),
                                      _lib.stream_ptr(device=masks.device)), "clasfv_lv_geometry")
    return LvCurve(area, geom)


def cleanup_masks(masks, label=1, holesize=128):
    """cleanupBinary of the reference (src/utils/camus_validate.py:284-352) for every frame, on the device, in
    one call: the 8-connected component of ``masks == label`` with the largest filled area is kept and its
    holes of fewer than ``holesize`` pixels (an integer in 1..32767) are filled; include/clasfv.h states the
    rule (clasfv_fuse_votes, CLASFV_FUSE_CLEAN). ``masks``: a device tensor (T,H,W) or (H,W) of an integer
    dtype, frames of at most 53248 pixels. Returns uint8 0/1 of the same shape on the masks' stream."""
    import torch
    from . import _lib
    if not torch.is_tensor(masks):
        raise ValueError("masks must be a tensor on the GPU (the library reads its device pointer)")
    if masks.is_floating_point() or masks.is_complex():
        raise ValueError(f"masks of an integer dtype expected, not {masks.dtype}")
    if masks.dim() not in (2, 3) or masks.numel() == 0:
        raise ValueError(f"masks (T,H,W) or (H,W) with at least one frame expected, got {tuple(masks.shape)}")
    h, w = masks.shape[-2:]
    _lib.check_clean_frame(h, w, "masks")
    method = _lib.FUSE_MAJORITY | _lib.clean_bits(holesize)
    if not masks.is_cuda:
        raise ValueError(f"masks must be on the GPU (the library reads their device pointer), not on {masks.device}")
    frames = (masks == label).to(torch.uint8).contiguous()  # K = 1: one pass's votes
    out = torch.empty_like(frames)
    t = frames.numel() // (h * w)
    lib = _lib.load()
    for at in range(0, t, 65535):  # majority takes at most 65535 output frames per call
        n = min(65535, t - at)
        src, dst = frames.view(-1, h, w)[at:at + n], out.view(-1, h, w)[at:at + n]
        _lib.check(lib.clasfv_fuse_votes(_lib.ptr(src), 1, n, 1, h, w, method, _lib.ptr(dst),
                                         _lib.stream_ptr(device=masks.device)), "clasfv_fuse_votes")
    return out


def ef_from_curve(area, volume, name, return_edes=False):
    """compute_ef_using_putative_clips from a per-frame curve (LvCurve.area, LvCurve.volume of one video;
    arrays or tensors): the same ED / ES pairs, EF = (V[ED] - V[ES]) / V[ED] * 100, negative EFs reported
    and dropped."""
    area, volume = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (area, volume))
    if area.ndim != 1 or area.shape != volume.shape:
        raise ValueError(f"area and volume of one video (T,) expected, got {area.shape} and {volume.shape}")
    pairs = ed_es_pairs(area)
    efs = []
    for d, s in pairs:
        with np.errstate(invalid="ignore", divide="ignore"):
            ef = (volume[d] - volume[s]) / volume[d] * 100
        if ef < 0:
            print("Negative EF at patient: " + str(name))
            continue
        efs.append(ef)
    return (efs, pairs) if return_edes else efs


def categorical_dice(prediction, truth, k, epsilon=1e-5):
    """Dice of class k (src/clasfv_losses.py:60-68), the parity metric: 2|A & B| / (|A| + |B| + eps)."""
    a = np.asarray(prediction) == k
    b = np.asarray(truth) == k
    return 2 * np.count_nonzero(a & b) / (np.count_nonzero(a) + np.count_nonzero(b) + epsilon)
