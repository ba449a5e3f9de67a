"""Motion-field warp on the HIP engine (``clasfv_warp``).

Reference semantics: ``generate_2dmotion_field`` (src/transform_utils.py:14-34) builds the sampling
grid x = linspace(-1,1,W)[j] + motion[:,0], y = linspace(-1,1,H)[i] + motion[:,1], and
``F.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=False)`` samples it
(src/visualization_utils.py:128, src/clasfv_losses.py:45,87). The kernel fuses both: the grid is
never materialised. ``track`` chains warps through the motion head's per-frame fields in one
``clasfv_track`` call and keeps every frame; ``apply_sequence_deformation``
(src/visualization_utils.py:107-130) is its last frame and ``track_labels`` the tracked mask video of
one labelled frame (:58-80).

``warp`` and bilinear ``track`` are differentiable: under autograd they run through
``clasfv_warp_backward`` (gradients of img and motion), which is what the training losses
(src/clasfv_losses.py:29-136, ``losses.py``) backpropagate through.
"""
import torch

from . import _lib


def _check(img, motion):
    """Refuses what the library would misread (it takes raw float32 device pointers): a host tensor, another
    dtype (never converted: a float64 image or the bf16 motion of an autocast region is the caller's to cast),
    two devices. Only strides are converted."""
    _lib.on_gpu(img, "img", dtype=torch.float32)
    _lib.on_gpu(motion, "motion", dtype=torch.float32)
    if motion.device != img.device:
        raise ValueError(f"img and motion must be on one GPU, not on {img.device} and {motion.device}")
    if img.dim() != 4 or motion.dim() != 4 or motion.shape[1] != 2:
        raise ValueError("img (N,C,H,W) and motion (N,2,H,W) expected")
    n, c, h, w = img.shape
    if tuple(motion.shape) != (n, 2, h, w):
        raise ValueError(f"motion shape {tuple(motion.shape)} does not match image {tuple(img.shape)}")
    if motion.stride(3) != 1 or motion.stride(2) != w:
        motion = motion.contiguous()
    return img.contiguous(), motion


def _warp_forward(img, motion, out=None):
    img, motion = _check(img, motion)
    n, c, h, w = img.shape
    if out is None:
        out = torch.empty_like(img)
    else:
        if not torch.is_tensor(out):
            raise TypeError(f"out= must be a torch tensor on {img.device}, not {type(out).__name__}")
        if (out.dtype != torch.float32 or out.shape != img.shape or out.device != img.device
                or not out.is_contiguous()):
            raise ValueError(f"out= must be a contiguous float32 tensor of img's shape {tuple(img.shape)} on {img.device}")
        for name, t in (("img", img), ("motion", motion)):  # every block reads both while others write out
            if _lib.overlap(out, t):
                raise ValueError(f"out= overlaps {name}: the warp cannot run in place")
    lib = _lib.load()
    _lib.check(lib.clasfv_warp(_lib.ptr(img), n, c, h, w, _lib.ptr(motion), motion.stride(0), motion.stride(1),
                               _lib.ptr(out), _lib.stream_ptr(device=img.device)), "clasfv_warp")
    return out


class _Warp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, motion):
        img, motion = _check(img, motion)
        ctx.save_for_backward(img, motion)
        return _warp_forward(img, motion)

    @staticmethod
    def backward(ctx, grad_out):
        img, motion = ctx.saved_tensors
        n, c, h, w = img.shape
        gimg = torch.zeros_like(img) if ctx.needs_input_grad[0] else None
        gmot = torch.empty((n, 2, h, w), device=img.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        if gimg is None and gmot is None:
            return None, None
        grad_out = grad_out.contiguous()
        lib = _lib.load()
        nul = _lib.ctypes.c_void_p(0)
        _lib.check(lib.clasfv_warp_backward(_lib.ptr(grad_out), _lib.ptr(img), n, c, h, w, _lib.ptr(motion),
                                            motion.stride(0), motion.stride(1),
                                            _lib.ptr(gimg) if gimg is not None else nul,
                                            _lib.ptr(gmot) if gmot is not None else nul,
                                            _lib.stream_ptr(device=img.device)),
                   "clasfv_warp_backward")
        return gimg, gmot


def warp(img, motion, out=None):
    """img (N,C,H,W) float32 on the device, motion (N,2,H,W) (any strides on N and the channel
    dim; H,W contiguous) -> warped (N,C,H,W) = grid_sample(img, generate_2dmotion_field(img, motion),
    bilinear, border, align_corners=False). Differentiable in img and motion. ``out`` (no autograd): a
    contiguous float32 tensor of img's shape on img's device to write into, overlapping neither img nor
    motion, else ValueError. img and motion must be float32 tensors on one GPU (ValueError; nothing is
    converted but strides); they may overlap each other."""
    for name, t in (("img", img), ("motion", motion)) + ((("out", out),) if out is not None else ()):
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a torch tensor on the GPU, not {type(t).__name__}")
    if torch.is_grad_enabled() and (img.requires_grad or motion.requires_grad):
        if out is not None:
            raise ValueError("out= is not supported under autograd")
        return _Warp.apply(img, motion)
    return _warp_forward(img, motion, out)


def generate_2dmotion_field(x, offset):
    """Reference-compatible grid (N,H,W,2) for callers that use F.grid_sample themselves."""
    n, _, h, w = x.shape
    gy, gx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    gx, gy = gx.to(offset.device), gy.to(offset.device)
    return torch.stack((gx[None] + offset[:, 0], gy[None] + offset[:, 1]), 3)


_MODES = {"bilinear": _lib.TRACK_BILINEAR, "nearest": _lib.TRACK_NEAREST}


def _check_track(img, motion, mode):
    if mode not in _MODES:
        raise ValueError(f"mode must be 'bilinear' or 'nearest', not {mode!r}")
    if img.dim() != 4 or motion.dim() != 5 or motion.shape[1] != 4:
        raise ValueError("img (N,C,H,W) and motion (N,4,T,H,W) expected")
    if img.dtype != torch.float32 or motion.dtype != torch.float32 or not img.is_cuda or motion.device != img.device:
        raise ValueError(f"img and motion must be float32 on one GPU (the library reads their device pointers), not "
                         f"{img.dtype} on {img.device} and {motion.dtype} on {motion.device}")
    n, c, h, w = img.shape
    if motion.shape[0] != n or tuple(motion.shape[3:]) != (h, w):
        raise ValueError(f"motion shape {tuple(motion.shape)} does not match image {tuple(img.shape)}")
    if motion.stride(4) != 1 or motion.stride(3) != w:
        motion = motion.contiguous()
    return img.contiguous(), motion


def _track_forward(img, motion, t0, t_step, count, forward, mode):
    """``count`` >= 1 chained warps in one clasfv_track call -> (count,N,C,H,W)."""
    n, c, h, w = img.shape
    out = torch.empty((count, n, c, h, w), device=img.device, dtype=torch.float32)
    pair = motion.data_ptr() + (0 if forward else 2) * motion.stride(1) * motion.element_size()
    lib = _lib.load()
    _lib.check(lib.clasfv_track(_lib.ptr(img), n, c, h, w, _lib.ctypes.c_void_p(pair), motion.stride(0),
                                motion.stride(1), motion.stride(2), motion.shape[2], t0, t_step, count, _MODES[mode],
                                _lib.ptr(out), _lib.stream_ptr(device=img.device)), "clasfv_track")
    return out


class _Track(torch.autograd.Function):
    """Bilinear ``track`` under autograd. The backward walks the chain in reverse with one
    clasfv_warp_backward per step (a fused backward kernel is out of scope)."""

    @staticmethod
    def forward(ctx, img, motion, t0, t_step, count, forward):
        img, motion = _check_track(img, motion, "bilinear")
        out = _track_forward(img, motion, t0, t_step, count, forward, "bilinear")
        ctx.save_for_backward(img, motion, out)
        ctx.chain = (t0, t_step, count, forward)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        img, motion, out = ctx.saved_tensors
        t0, t_step, count, forward = ctx.chain
        want_img, want_mot = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_img or want_mot):
            return None, None, None, None, None, None
        n, c, h, w = img.shape
        ch = 0 if forward else 2
        grad_out = grad_out.contiguous()
        gmotion = torch.zeros(motion.shape, device=img.device, dtype=torch.float32) if want_mot else None
        gstep = torch.empty((n, 2, h, w), device=img.device, dtype=torch.float32) if want_mot else None
        lib = _lib.load()
        nul = _lib.ctypes.c_void_p(0)
        g = grad_out[count - 1]   # d loss / d out[p], complete once step p + 1 has added its share
        for p in range(count - 1, -1, -1):
            t = t0 + p * t_step
            src = out[p - 1] if p else img
            mot = motion[:, ch:ch + 2, t]
            need_src = p > 0 or want_img   # the first step's source is img itself
            gsrc = torch.zeros_like(img) if need_src else None
            _lib.check(lib.clasfv_warp_backward(_lib.ptr(g), _lib.ptr(src), n, c, h, w, _lib.ptr(mot), mot.stride(0),
                                                mot.stride(1), _lib.ptr(gsrc) if need_src else nul,
                                                _lib.ptr(gstep) if want_mot else nul,
                                                _lib.stream_ptr(device=img.device)), "clasfv_warp_backward")
            if want_mot:
                gmotion[:, ch:ch + 2, t] = gstep
            g = gsrc + grad_out[p - 1] if p else gsrc
        return (g if want_img else None), gmotion, None, None, None, None


def track(img, motion, start_index, end_index, forward=True, mode="bilinear"):
    """Push one frame img (N,C,H,W) through motion (N,4,T,H,W) frames ``range(start_index, end_index,
    +1 if forward else -1)``, forward fields (channels 0,1) or backward (2,3), and keep every frame:
    returns (P,N,C,H,W), frame p the image after p + 1 warps (what the reference's
    apply_sequence_deformation returns for end_index = start_index +- (p + 1)). One ``clasfv_track``
    call; an empty range gives an empty (0,N,C,H,W) tensor. mode "bilinear" (images, one-hot labels;
    differentiable in img and motion) or "nearest" (label maps; ValueError under autograd)."""
    t_step = 1 if forward else -1
    count = len(range(start_index, end_index, t_step))
    img, motion = _check_track(img, motion, mode)
    if count == 0:
        return torch.empty((0,) + tuple(img.shape), device=img.device, dtype=torch.float32)
    if torch.is_grad_enabled() and (img.requires_grad or motion.requires_grad):
        if mode != "bilinear":
            raise ValueError("mode='nearest' is piecewise constant: not supported under autograd")
        return _Track.apply(img, motion, start_index, t_step, count, forward)
    return _track_forward(img, motion, start_index, t_step, count, forward, mode)


def apply_sequence_deformation(img, motion, start_index, end_index, forward=True, grid_mode="bilinear"):
    """Recursively warp one frame img (N,C,H,W) through motion (N,4,T,H,W) frames
    start_index..end_index (exclusive), forward fields (channels 0,1) or backward (2,3);
    grid_mode "bilinear" or "nearest" as the reference's. The last frame of ``track``; img itself for
    an empty range."""
    frames = track(img, motion, start_index, end_index, forward, grid_mode)
    return frames[-1] if frames.shape[0] else img.contiguous()


def track_labels(labels, motion, seed_index):
    """Tracked mask video from one labelled frame: labels (N,T,H,W) integer (|label| < 2^24) and motion
    (N,4,T,H,W) on the device -> int64 (N,T,H,W). Frame seed_index is labels[:, seed_index]; the frames
    after it are that frame pushed through the forward fields (the chain at frame f uses
    motion[:, :2, f] and lands on f + 1), the frames before it through the backward fields
    (motion[:, 2:, f], landing on f - 1), both in nearest mode (get_deformed_label_forback,
    src/visualization_utils.py:58-80). Only the seed frame of ``labels`` is read."""
    if labels.dim() != 4 or labels.is_floating_point() or labels.is_complex():
        raise ValueError("labels (N,T,H,W) of an integer dtype expected")
    n, t, h, w = labels.shape
    if not labels.is_cuda:
        raise ValueError(f"labels must be on the GPU, not on {labels.device}")
    if not 0 <= seed_index < t or motion.dim() != 5 or motion.shape[2] != t:
        raise ValueError(f"seed_index {seed_index} or motion {tuple(motion.shape)} does not match labels "
                         f"{tuple(labels.shape)}")
    seed = labels[:, seed_index].to(torch.float32).unsqueeze(1)
    out = torch.empty((n, t, h, w), device=labels.device, dtype=torch.int64)
    out[:, seed_index] = labels[:, seed_index]
    with torch.no_grad():
        after = track(seed, motion, seed_index, t - 1, forward=True, mode="nearest")
        before = track(seed, motion, seed_index, 0, forward=False, mode="nearest")
    out[:, seed_index + 1:] = after[:, :, 0].permute(1, 0, 2, 3)
    out[:, :seed_index] = before[:, :, 0].permute(1, 0, 2, 3).flip(1)
    return out
