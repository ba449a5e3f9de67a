"""The annotated LV video of the reference's ``make_annotated_gif`` (src/visualization_utils.py:476-539),
rendered on the device: overlay pane, title band and volume-curve strip of every frame in one kernel
(clasfv_render_annotated; include/clasfv.h states the rules pixel for pixel). Only finished frames go back
to the host, where ``write_gif`` hands them to PIL.
"""
import numpy as np

from . import _lib

SIZE, TITLE_HEIGHT, STRIP_HEIGHT = 553, 40, 80  # the reference's geometry: a 553-wide frame of 553 + 40 + 80 rows
THICKNESS = 2.0                                  # pixels; matplotlib's default 1.5 pt line at 100 dpi
LIME = (50, 205, 50)
TITLE = "LV Volume (ml)"
MAX_BYTES = 2 ** 32 - 1                          # of one clasfv_render_annotated call
_TITLES = {}


def title_band(height=TITLE_HEIGHT, width=SIZE):
    """(height, width, 3) uint8: "LV Volume (ml)" in lime green on black, PIL's built-in bitmap font scaled
    by a whole factor and centred; a black band without PIL. Made once per size. Presentation only."""
    key = (int(height), int(width))
    if key not in _TITLES:
        band = np.zeros(key + (3,), np.uint8)
        try:
            from PIL import Image, ImageDraw, ImageFont
        except ImportError:
            Image = None
        if Image is not None and key[0] > 0:
            font = ImageFont.load_default()
            x0, y0, x1, y1 = ImageDraw.Draw(Image.new("RGB", (1, 1))).textbbox((0, 0), TITLE, font=font)
            text = Image.new("RGB", (max(1, x1), max(1, y1)))
            ImageDraw.Draw(text).text((0, 0), TITLE, fill=LIME, font=font)
            text = text.crop((x0, y0, x1, y1))
            k = max(1, min((key[0] - 4) // max(1, text.height), (key[1] - 4) // max(1, text.width)))
            text = text.resize((text.width * k, text.height * k), Image.NEAREST)
            img = Image.fromarray(band)
            img.paste(text, ((key[1] - text.width) // 2, (key[0] - text.height) // 2))
            band = np.asarray(img, np.uint8).copy()
        _TITLES[key] = band
    return _TITLES[key]


def annotate_video(video, masks, volume=None, truth=None, size=SIZE, title=True, first=0, count=None, label=1,
                   title_height=TITLE_HEIGHT, strip_height=STRIP_HEIGHT, thickness=THICKNESS, pane_height=None):
    """Frames [first, first + count) of the annotated video -> uint8 device tensor
    (count, pane_height + Ht + Hs, size, 3), on the inputs' device and current stream.

    ``video`` (3,T,H,W) float32, normalised to [0, 1]; ``masks`` (T,H,W) of an integer dtype (uint8 is read in
    place, others are compared with ``label`` on the device first, as echo.lv_curve does); ``truth`` the same
    (optional: the pane becomes the reference's difference image). ``volume``: T float64 volumes on the device,
    or None for ``echo.lv_curve(masks).volume``, read in place. ``title``: True for the cached "LV Volume (ml)"
    band, False / None for a black one, or a (title_height, size, 3) uint8 image. ``pane_height`` defaults to
    ``size`` (the reference's square pane). Ht = ``title_height``, Hs = ``strip_height``."""
    import torch
    from . import echo
    for name, t in (("video", video), ("masks", masks)) + ((("truth", truth),) if truth is not None else ()):
        if not torch.is_tensor(t):
            raise ValueError(f"{name} must be a tensor on the GPU (the library reads its device pointer)")
    if video.dim() != 4 or video.shape[0] != 3 or video.numel() == 0 or video.dtype != torch.float32:
        raise ValueError(f"video (3,T,H,W) float32 expected, got {tuple(video.shape)} {video.dtype}")
    _, T, H, W = video.shape
    for name, t in (("masks", masks), ("truth", truth)):
        if t is not None and tuple(t.shape) != (T, H, W):
            raise ValueError(f"{name} {(T, H, W)} expected (the video's frames), got {tuple(t.shape)}")
        if t is not None and (t.is_floating_point() or t.is_complex()):
            raise ValueError(f"{name} of an integer dtype expected, not {t.dtype}")
    if int(label) != label or not 0 <= label <= 255:
        raise ValueError(f"label {label!r} must be an integer in [0, 255]")
    hp = size if pane_height is None else pane_height
    for name, v, least in (("size", size, 1), ("pane_height", hp, 1), ("title_height", title_height, 0),
                           ("strip_height", strip_height, 0)):
        if int(v) != v or v < least:
            raise ValueError(f"{name} must be an integer >= {least}, got {v!r}")
    wo, hp, ht, hs = int(size), int(hp), int(title_height), int(strip_height)
    count = T - first if count is None else count
    if int(first) != first or int(count) != count or first < 0 or count < 1 or first + count > T:
        raise ValueError(f"frames [first, first + count) = [{first}, {first}+{count}) must lie in [0, {T})")
    thickness = float(thickness)
    if not (np.isfinite(thickness) and thickness >= 0):
        raise ValueError(f"thickness must be finite and not negative, got {thickness!r}")
    frame_bytes = (hp + ht + hs) * wo * 3
    if frame_bytes > MAX_BYTES or H * W >= 2 ** 31:
        raise ValueError(f"a frame of {frame_bytes} bytes (at most {MAX_BYTES}) or a source of {H} x {W} pixels is "
                         f"past what the kernel addresses")
    if not video.is_cuda:
        raise ValueError(f"video must be on the GPU (the library reads its device pointer), not on {video.device}")
    dev = video.device
    for name, t in (("masks", masks), ("truth", truth)):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} must be on the video's device {dev}, not on {t.device}")
    video = video.contiguous()
    if masks.dtype == torch.uint8 and (truth is None or truth.dtype == torch.uint8):
        m8, t8, lab = masks.contiguous(), (truth.contiguous() if truth is not None else None), int(label)
    else:  # compared with the label on the device first; the library reads dense (T,H,W) uint8 blocks
        m8 = (masks == label).to(torch.uint8).contiguous()
        t8 = (truth == label).to(torch.uint8).contiguous() if truth is not None else None
        lab = 1
    if volume is None:
        geom = echo.lv_curve(m8, lab).geom  # (T, 12): the volume is element 11 of every row
        vol, vptr, vstride = geom, geom.data_ptr() + 8 * (_lib.LV_STRIDE - 1), _lib.LV_STRIDE
    else:
        vol = torch.as_tensor(volume, dtype=torch.float64).to(dev)
        if vol.dim() != 1 or vol.shape[0] != T:
            raise ValueError(f"volume: {T} values expected (one per frame), got {tuple(vol.shape)}")
        if T > 1 and vol.stride(0) < 1:
            vol = vol.contiguous()
        vptr, vstride = vol.data_ptr(), (vol.stride(0) if T > 1 else 1)
    band = None
    if title is True:
        band = torch.from_numpy(title_band(ht, wo)).to(dev) if ht else None
    elif title is not None and title is not False:
        band = torch.as_tensor(title).to(dev)
        if tuple(band.shape) != (ht, wo, 3) or band.dtype != torch.uint8:
            raise ValueError(f"title ({ht}, {wo}, 3) uint8 expected, got {tuple(band.shape)} {band.dtype}")
        band = band.contiguous() if ht else None
    lib = _lib.load()
    out = torch.empty((count, hp + ht + hs, wo, 3), dtype=torch.uint8, device=dev)
    work = torch.empty(int(lib.clasfv_render_workspace_bytes()) // 8, dtype=torch.float64, device=dev)
    per_call = max(1, MAX_BYTES // frame_bytes)  # chunks of frames give the bytes of one call
    for f0 in range(0, count, per_call):
        n = min(per_call, count - f0)
        _lib.check(lib.clasfv_render_annotated(
            _lib.ptr(video), _lib.ptr(m8), _lib.ptr(t8) if t8 is not None else None, T, H, W, vptr, vstride,
            _lib.ptr(band) if band is not None else None, first + f0, n, hp, wo, ht, hs, lab, thickness,
            _lib.ptr(work), _lib.ptr(out[f0]), _lib.stream_ptr(device=dev)), "clasfv_render_annotated")
    return out


def write_gif(frames, path, fps=30):
    """(N,H,W,3) uint8 frames (array or tensor) -> an endlessly looping GIF through PIL."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError(f"{path}: PIL (Pillow) is not installed, so no GIF can be written; save the frames "
                           f"instead (numpy.save(<name>.npy, frames), what the CLI does)") from e
    frames = np.ascontiguousarray(frames.cpu().numpy() if hasattr(frames, "cpu") else frames, dtype=np.uint8)
    if frames.ndim != 4 or frames.shape[-1] != 3 or len(frames) < 1:
        raise ValueError(f"frames (N,H,W,3) expected, got {frames.shape}")
    images = [Image.fromarray(f) for f in frames]
    images[0].save(path, format="GIF", save_all=True, append_images=images[1:], duration=max(1, round(1000 / fps)),
                   loop=0)
    return path


def make_annotated_gif(segmentations, video, filename="example.gif"):
    """The reference's make_annotated_gif: ``segmentations`` (T,H,W) labels and the normalised ``video``
    (3,T,H,W), arrays or tensors, to an annotated GIF at ``filename``."""
    import torch
    dev = next((t.device for t in (video, segmentations) if torch.is_tensor(t) and t.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))
    seg = torch.as_tensor(np.asarray(segmentations) if not torch.is_tensor(segmentations) else segmentations).to(dev)
    vid = torch.as_tensor(np.asarray(video) if not torch.is_tensor(video) else video).to(dev, torch.float32)
    return write_gif(annotate_video(vid, seg), filename)
