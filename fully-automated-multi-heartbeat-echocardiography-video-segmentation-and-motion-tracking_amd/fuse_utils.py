"""Drop-in clip plumbing and label fusion (src/fuse_utils.py:16-100) on the HIP engine.

``segment_a_video_with_fusion(video, model, interpolate_last=True, step=1, num_clips=10,
fuse_method="simple", class_list=[0, 1])`` returns the same (T', 112, 112) int64 label video as the
reference, but every clip of every temporally shifted pass is built on the GPU
(``clasfv_build_clips``), run through the model in batches instead of one batch-1 forward per clip
(src/fuse_utils.py:53-61), and softmax -> temporal re-interpolation -> argmax -> per-frame fusion
stay in HBM (``clasfv_pass_labels``, ``clasfv_fuse_votes``); only the final uint8 mask crosses PCIe.

Reference behaviour kept: banker's rounding of the clip count (:22,29), the K clamp and its
"Video is too short" message (:38-42), passes with different clip counts (numpy 1.19 ragged arrays,
:50). Two reference quirks are reproduced by default (``strict_reference=True``) and corrected with
``strict_reference=False``: K == 0 after the clamp (T in [32, 32 + step), e.g. a single 32-frame
clip) raises IndexError at :82 -- non-strict runs the one unshifted pass; frames 1..step-1 are
dropped for step > 1 (:85) -- non-strict keeps them with their single (pass 0) vote, so the output
always has T frames.
Fusion: ``majority`` (= ``majorityvoting``/``mv``; ties -> background), ``itkvoting`` (= ``voting``;
itk::LabelVotingImageFilter with its default undecided label: ties -> 2), ``simple`` (SIMPLE,
Langerak 2010) and ``staple`` (STAPLE, Warfield 2004), up to 64 passes. LabelFusion itself is not
available, so every rule but ``majority`` (pinned by the reference-run goldens of its stub) is
parity-unpinned.
``cleanup=True`` (with ``holesize``) on ``fuse_votes`` and the two segment functions cleans every fused frame in
the fusion call: the reference's cleanupBinary (src/utils/camus_validate.py:284-352) on the device
(CLASFV_FUSE_CLEAN, include/clasfv.h), parity-unpinned as well.
"""
import numpy as np
import torch

from . import _lib

FUSE_METHODS = {"majority": _lib.FUSE_MAJORITY, "majorityvoting": _lib.FUSE_MAJORITY, "mv": _lib.FUSE_MAJORITY,
                "itkvoting": _lib.FUSE_ITKVOTING, "voting": _lib.FUSE_ITKVOTING, "simple": _lib.FUSE_SIMPLE,
                "staple": _lib.FUSE_STAPLE}
MAX_PASSES = 64  # CLASFV_MAX_PASSES
CLIP = 32
DEFAULT_BATCH = 32


def n_clips(t, clip_length=CLIP):
    """Number of clips of a t-frame video: round(t / 32) with numpy's half-to-even rounding."""
    return int(np.round(t / clip_length))


def clamp_num_clips(t, num_clips, step, strict_reference=True):
    """src/fuse_utils.py:38-42. The reference can clamp to K == 0 (T in [32, 32 + step)), which then
    fails at :82; with strict_reference=False that case runs the one unshifted pass instead."""
    if t < CLIP + num_clips * step:
        num_clips = (t - CLIP) // step
    if num_clips < 0:
        print("Video is too short")
        num_clips = 1
    if num_clips == 0 and not strict_reference:
        num_clips = 1
    return num_clips


def fused_frames(t, step, strict_reference=True):
    """Frames of the fused output: the reference drops frames 1..step-1 (src/fuse_utils.py:85)."""
    return t if not strict_reference else t - (step - 1)


def keep_dropped_frames(labels, fused, step):
    """Non-strict output: the strict fused video (frames 0, step, step+1, ...) with frames 1..step-1
    re-inserted. Those frames have a single vote -- pass 0's label, as the reference's own loop would
    give them if it did not skip them (:85-93)."""
    if step == 1:
        return fused
    return torch.cat([fused[:1], labels[0, 1:step].to(fused.dtype), fused[1:]])


def clip_table(t, num_passes, step, interpolate_last=True):
    """[(shift, first_frame)] for every clip of every shifted pass, pass-major; and per-pass offsets."""
    table, clip0 = [], []
    for k in range(num_passes):
        shift = k * step
        tk = t - shift
        nk = n_clips(tk)
        if tk % CLIP != 0 and not interpolate_last and nk * CLIP > tk:
            raise ValueError("all the input array dimensions except for the concatenation axis must match exactly")
        if nk == 0:
            raise ValueError(f"pass {k}: {tk} frames give no 32-frame clip")
        clip0.append(len(table))
        table.extend((shift, CLIP * j) for j in range(nk))
    return table, clip0


def _device_of(model):
    eng = getattr(model, "engine", None)
    if eng is not None:
        return eng.device
    return torch.device("cuda", torch.cuda.current_device())


def to_device_video(video, device):
    v = torch.as_tensor(np.asarray(video, np.float32) if not torch.is_tensor(video) else video)
    return v.to(device, torch.float32).contiguous()


_TABLES = {}


def check_clip_table(table, t, interpolate_last=True):
    """ValueError unless every (shift, first_frame) of a clip table names 32 frames that clasfv_build_clips
    can read from a t-frame video: 0 <= shift < t, first_frame >= 0, and first_frame + 32 within the pass's
    length -- 32 * n_clips(t - shift) when the pass is resampled (interpolate_last and (t - shift) % 32 != 0),
    else t - shift. The kernel trusts the table; an entry past that reads out of bounds."""
    for i, entry in enumerate(table):
        try:
            shift, first = entry
            ok = int(shift) == shift and int(first) == first
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"table[{i}] = {entry!r}: a pair of integers (shift, first_frame) expected")
        if not 0 <= shift < t:
            raise ValueError(f"table[{i}]: shift {shift} outside [0, {t}) of the {t}-frame video")
        tk = t - shift
        length = CLIP * n_clips(tk) if interpolate_last and tk % CLIP != 0 else tk
        if first < 0 or first + CLIP > length:
            raise ValueError(f"table[{i}]: frames [{first}, {first} + {CLIP}) outside the pass's {length} frames "
                             f"(shift {shift}, {t}-frame video)")


def _device_table(table, device, t=None, interpolate_last=True):
    """Device int32 copy of a clip table, cached: a fresh pageable host->device copy per call would
    make every video wait for the copy engine (and the host for the stream) before its clips build.
    A table is allocated on the stream that first asked for it and read by kernels on every stream that
    asks later, so each hand-out records the current stream on it: when the cache is emptied, the
    allocator keeps the block until the work queued on those streams so far has run (without that, a new
    tensor could take the block while a kernel that has not started yet still reads the table).
    With ``t`` (the video's frames) the host list is checked against it (check_clip_table) before it is
    uploaded, on a cache miss only: the key holds t and interpolate_last, so a hit was checked for them.
    Without ``t`` nothing is checked and the key has no t: the package never calls it so; the form is kept for
    callers that upload a table of their own making and answer for it (the cache-eviction test does)."""
    key = (str(device), tuple(table)) if t is None else (str(device), tuple(table), t, bool(interpolate_last))
    tab = _TABLES.get(key)
    if tab is None:
        if t is not None:
            check_clip_table(key[1], t, interpolate_last)
        if len(_TABLES) > 256:
            _TABLES.clear()
        tab = torch.tensor(np.asarray(key[1], np.int32).reshape(-1), device=device)
        _TABLES[key] = tab
    tab.record_stream(torch.cuda.current_stream(tab.device))
    return tab


def build_clips(video_dev, table, interpolate_last=True):
    """(n,3,32,H,W) clips on the device for a [(shift, first_frame)] table. ``video_dev``: a (3,T,H,W)
    tensor on the GPU (any dtype and strides: converted); every table entry must lie inside the shifted,
    resampled video (check_clip_table), else ValueError."""
    _lib.on_gpu(video_dev, "video_dev")
    if video_dev.dim() != 4 or video_dev.shape[0] != 3:
        raise ValueError(f"video_dev: expected a (3,T,H,W) video, got {tuple(video_dev.shape)}")
    _, t, h, w = video_dev.shape
    tab = _device_table(table, video_dev.device, t, interpolate_last)  # a bad table is refused before any copy
    video_dev = video_dev.to(torch.float32).contiguous()  # the ABI takes dense row-major buffers
    clips = torch.empty((len(table), 3, CLIP, h, w), device=video_dev.device, dtype=torch.float32)
    lib = _lib.load()
    _lib.check(lib.clasfv_build_clips(_lib.ptr(video_dev), t, h, w, _lib.ptr(tab), len(table), int(bool(interpolate_last)),
                                      _lib.ptr(clips), _lib.stream_ptr(device=video_dev.device)), "clasfv_build_clips")
    return clips


def divide_to_consecutive_clips(video, clip_length=CLIP, interpolate_last=False):
    """src/fuse_utils.py:16-33. Returns a float32 device tensor (n,3,32,H,W)."""
    if clip_length != CLIP:
        raise ValueError("the engine uses 32-frame clips")
    dev = torch.device("cuda", torch.cuda.current_device())
    v = to_device_video(video, dev)
    table, _ = clip_table(v.shape[1], 1, 1, interpolate_last)
    return build_clips(v, table, interpolate_last)


def run_model(model, clips, batch_size=None, return_motion=False):
    """Segmentation logits (n,2,32,H,W) of every clip. By default the motion output is discarded as in the
    reference (src/fuse_utils.py:59); ``return_motion=True`` returns ``(logits, motion)`` with the motion
    fields (n,4,32,H,W) float32 of the same forwards (beats.track_beats tracks through them)."""
    n = clips.shape[0]
    if batch_size is None:
        batch_size = DEFAULT_BATCH if hasattr(model, "engine") else 1
    outs, mots = [], []
    for s in range(0, n, batch_size):
        seg, mot = model(clips[s:s + batch_size])
        outs.append(seg.to(clips.device, torch.float32))
        if return_motion:
            mots.append(mot.to(clips.device, torch.float32))
    join = lambda xs: torch.cat(xs) if len(xs) > 1 else xs[0].contiguous()
    return (join(outs), join(mots)) if return_motion else join(outs)


def check_fuse_votes_args(shape, step):
    """ValueError unless (K,T,H,W) = ``shape`` and ``step`` are what clasfv_fuse_votes takes. Host arithmetic."""
    if len(shape) != 4:
        raise ValueError(f"labels (K,T,H,W) expected, got {tuple(shape)}")
    k, t = shape[0], shape[1]
    if not 1 <= k <= MAX_PASSES:
        raise ValueError(f"labels: 1 to {MAX_PASSES} shifted passes are supported (got K = {k})")
    if isinstance(step, bool) or int(step) != step or step < 1 or t - (step - 1) < 1:
        raise ValueError(f"step {step!r} must be an integer >= 1 that leaves T - (step - 1) >= 1 of the {t} frames")


def check_pass_labels_args(shape, clip0, t, step, margin=False):
    """ValueError unless logits of ``shape`` hold every clip that clasfv_pass_labels reads for the passes
    ``clip0``, ``t`` frames and ``step`` (pass k: clips [clip0[k], clip0[k] + n_clips(t - k * step))); returns
    that clip count. Host arithmetic."""
    k = len(clip0)
    if k > MAX_PASSES:
        raise ValueError(f"clip0: at most {MAX_PASSES} shifted passes are supported (got {k})")
    want = (CLIP,) if margin else (2, CLIP)
    if len(shape) != len(want) + 3 or tuple(shape[1:-2]) != want:
        raise ValueError(f"logits (n,{','.join(map(str, want))},H,W) expected{' with margin=True' if margin else ''}, "
                         f"got {tuple(shape)}")
    if int(t) != t or int(step) != step or not 1 <= t <= 65535 or step < 1 or (k - 1) * step >= t:
        raise ValueError(f"t = {t!r} frames (1 to 65535) and step = {step!r} (>= 1) must leave every one of the {k} "
                         f"passes a frame")
    need = 0
    for j, c0 in enumerate(clip0):
        if int(c0) != c0 or c0 < 0:
            raise ValueError(f"clip0[{j}] = {c0!r}: the pass's first clip, an integer >= 0, expected")
        need = max(need, c0 + n_clips(t - j * step))
    if shape[0] < need:
        raise ValueError(f"logits holds {shape[0]} clips, but the passes read {need} (clip0 {list(clip0)}, "
                         f"{t} frames, step {step})")
    return need


def fuse_votes(labels, step, fuse_method="simple", force_generic=False, cleanup=False, holesize=128):
    """Per-frame fusion of (K,T,H,W) uint8 pass labels -> (T-(step-1),H,W) uint8. ``force_generic``
    runs SIMPLE on its generic kernel instead of the packed <= 16-vote one (A/B tests). ``labels``: on the
    GPU (any integer dtype and strides: converted), K <= 64; ``step`` >= 1 with T - (step - 1) >= 1.
    ``cleanup=True`` cleans every fused frame in the same call (CLASFV_FUSE_CLEAN, include/clasfv.h: the label-1
    component of largest filled area is kept and its holes below ``holesize`` pixels, an integer in 1..32767,
    are filled); frames of at most 53248 pixels."""
    _lib.on_gpu(labels, "labels")
    check_fuse_votes_args(labels.shape, step)
    k, t, h, w = labels.shape
    clean = 0
    if cleanup:
        clean = _lib.clean_bits(holesize)
        _lib.check_clean_frame(h, w, "labels")
    labels = labels.to(torch.uint8).contiguous()
    method = FUSE_METHODS.get(fuse_method.lower())
    if method is None:
        raise NotImplementedError(f"fuse_method {fuse_method!r}: supported {sorted(FUSE_METHODS)}")
    if force_generic:
        method |= _lib.FUSE_FORCE_GENERIC
    method |= clean
    fused = torch.empty((t - (step - 1), h, w), device=labels.device, dtype=torch.uint8)
    lib = _lib.load()
    _lib.check(lib.clasfv_fuse_votes(_lib.ptr(labels), k, t, step, h, w, method, _lib.ptr(fused),
                                     _lib.stream_ptr(device=labels.device)), "clasfv_fuse_votes")
    return fused


def ctypes_int32_array(vals):
    """Host int32 array for the ABI; returns (pointer, owner) -- keep the owner alive for the call."""
    import ctypes
    arr = (ctypes.c_int32 * max(1, len(vals)))(*vals)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def segment_a_video_with_fusion_device(video, model, interpolate_last=True, step=1, num_clips=10, fuse_method="simple",
                                       class_list=(0, 1), batch_size=None, strict_reference=True, cleanup=False,
                                       holesize=128):
    """Same as segment_a_video_with_fusion but returns the fused (T',H,W) uint8 mask on the device."""
    if list(class_list) != [0, 1]:
        raise ValueError("the engine fuses the two CLAS-FV classes [0, 1]")
    if cleanup:
        _lib.clean_bits(holesize)  # refused before any device work
    dev = _device_of(model)
    v = to_device_video(video, dev)
    t = v.shape[1]
    k = clamp_num_clips(t, num_clips, step, strict_reference)
    if k == 0:
        raise IndexError("list index out of range")  # src/fuse_utils.py:82 with no pass
    table, clip0 = clip_table(t, k, step, interpolate_last)
    clips = build_clips(v, table, interpolate_last)
    logits = run_model(model, clips, batch_size)
    labels = pass_labels(logits, clip0, t, step, interpolate_last)
    fused = fuse_votes(labels, step, fuse_method, cleanup=cleanup, holesize=holesize)
    if strict_reference:
        return fused
    if not cleanup or step == 1:
        return keep_dropped_frames(labels, fused, step)
    # pass 0's frames 1..step-1, re-inserted with their single vote, are cleaned like the fused ones
    kept = fuse_votes(labels[:1, 1:step], 1, "majority", cleanup=True, holesize=holesize)
    return torch.cat([fused[:1], kept, fused[1:]])


def logit_margin(logits):
    """(n,2,32,H,W) logits on the GPU (any dtype and strides: converted) -> (n,32,H,W) margins l1 - l0
    (what pass_labels(margin=True) consumes)."""
    _lib.on_gpu(logits, "logits")
    if logits.dim() != 5 or logits.shape[1] != 2 or logits.shape[2] != CLIP:
        raise ValueError(f"logits (n,2,{CLIP},H,W) expected, got {tuple(logits.shape)}")
    logits = logits.to(torch.float32).contiguous()
    n, _, c, h, w = logits.shape
    out = torch.empty((n, c, h, w), device=logits.device, dtype=torch.float32)
    lib = _lib.load()
    _lib.check(lib.clasfv_logit_margin(_lib.ptr(logits), n, h, w, _lib.ptr(out), _lib.stream_ptr(device=logits.device)),
               "clasfv_logit_margin")
    return out


def pass_labels(logits, clip0, t, step, interpolate_last=True, margin=False):
    """(K,T,H,W) uint8 labels of the K shifted passes (softmax -> resample -> argmax). ``logits``
    is (n,2,32,H,W), or (n,32,H,W) margins l1 - l0 with ``margin=True`` (bit-identical labels), on the GPU
    (any dtype and strides: converted). Pass k reads clips [clip0[k], clip0[k] + n_clips(t - k * step)) of it:
    ``logits`` must hold them all, else ValueError (the kernel takes K, clip0 and T on trust)."""
    _lib.on_gpu(logits, "logits")
    check_pass_labels_args(logits.shape, clip0, t, step, margin)
    k = len(clip0)
    logits = logits.to(torch.float32).contiguous()
    h, w = logits.shape[-2:]
    labels = torch.empty((k, t, h, w), device=logits.device, dtype=torch.uint8)
    ptr, keep = ctypes_int32_array(clip0)
    lib = _lib.load()
    fn = lib.clasfv_pass_labels_margin if margin else lib.clasfv_pass_labels
    _lib.check(fn(_lib.ptr(logits), k, ptr, t, step, h, w, int(bool(interpolate_last)), _lib.ptr(labels),
                  _lib.stream_ptr(device=logits.device)), "clasfv_pass_labels")
    del keep
    return labels


def segment_a_video_with_fusion(video, model, interpolate_last=True, step=1, num_clips=10, fuse_method="simple",
                                class_list=[0, 1], batch_size=None, strict_reference=True, cleanup=False, holesize=128):
    """src/fuse_utils.py:36-100 -> numpy int64 (T', H, W). ``strict_reference=False`` corrects the
    two reference quirks (see the module docstring): T' == T always, and T == 32 yields masks.
    ``cleanup=True``: every returned frame is cleaned on the device (fuse_votes' ``cleanup``, ``holesize``)."""
    fused = segment_a_video_with_fusion_device(video, model, interpolate_last, step, num_clips, fuse_method, class_list,
                                               batch_size, strict_reference, cleanup, holesize)
    return fused.to(torch.int64).cpu().numpy()
