"""ctypes binding of ``libclasfv.so`` (C ABI declared in include/clasfv.h).

There is no CPU fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
import ctypes
import numbers
import os

from .build import LIB_PATH

c_int, c_int64, c_void_p, c_char_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_char_p
_P = c_void_p

PLAN_MAX_RANGES = 8  # CLASFV_PLAN_MAX_RANGES
# CLASFV_PLAN_* kinds, range roles and the caller's tensors' buffer ids (include/clasfv.h)
PLAN_KINDS = ("pack", "conv", "split_sum", "dec_index", "decoder", "fork", "join")
PLAN_ROLES = ("x", "x2", "res", "y", "part", "idx", "tap")
PLAN_EXTERNAL = {-1: "clip", -2: "seg", -3: "motion"}


class PlanRange(ctypes.Structure):  # clasfv_plan_range_t
    _fields_ = [("buffer", ctypes.c_int32), ("role", ctypes.c_int32), ("write", ctypes.c_int32), ("pad_", ctypes.c_int32),
                ("offset", c_int64), ("bytes", c_int64)]


class PlanLaunch(ctypes.Structure):  # clasfv_plan_launch_t
    _fields_ = [("sub_batch", ctypes.c_int32), ("stream", ctypes.c_int32), ("kind", ctypes.c_int32),
                ("conv", ctypes.c_int32), ("kernel", c_char_p), ("split_asked", ctypes.c_int32),
                ("split_granted", ctypes.c_int32), ("x_c8", ctypes.c_int32), ("y_c8", ctypes.c_int32),
                ("relu", ctypes.c_int32), ("has_res", ctypes.c_int32), ("x_elem", ctypes.c_int32),
                ("y_elem", ctypes.c_int32), ("n_ranges", ctypes.c_int32), ("pad_", ctypes.c_int32),
                ("range", PlanRange * PLAN_MAX_RANGES)]


class PlanBuffer(ctypes.Structure):  # clasfv_plan_buffer_t
    _fields_ = [("sub_batch", ctypes.c_int32), ("clips", ctypes.c_int32), ("id", ctypes.c_int32), ("pad_", ctypes.c_int32),
                ("name", c_char_p), ("offset", c_int64), ("bytes", c_int64), ("total", c_int64)]


# name -> (restype, argtypes); mirrors include/clasfv.h
SIGNATURES = {
    "clasfv_last_error": (c_char_p, []),
    "clasfv_version": (c_int, []),
    "clasfv_source_hash": (c_char_p, []),
    "clasfv_create": (c_int, [c_int, ctypes.POINTER(c_void_p)]),
    "clasfv_destroy": (c_int, [_P]),
    "clasfv_param_count": (c_int, [_P]),
    "clasfv_param_info": (c_int, [_P, c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_int), ctypes.POINTER(c_int64)]),
    "clasfv_load_param": (c_int, [_P, c_char_p, _P, c_int64]),
    "clasfv_finalize": (c_int, [_P]),
    "clasfv_forward": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "clasfv_workspace_bytes": (c_int64, [_P]),
    "clasfv_max_clips": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "clasfv_clips_fit": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "clasfv_set_compute_dtype": (c_int, [_P, c_int]),
    "clasfv_get_compute_dtype": (c_int, [_P]),
    "clasfv_set_kernel_variants": (c_int, [_P, c_int]),
    "clasfv_get_kernel_variants": (c_int, [_P]),
    "clasfv_set_kernel_timing": (c_int, [_P, c_int]),
    "clasfv_kernel_timing": (c_int, [_P, c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_int),
                                     ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(ctypes.c_double)]),
    "clasfv_set_launch_log": (c_int, [_P, c_int]),
    "clasfv_launch_log": (c_int, [_P, c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_int64), ctypes.POINTER(c_int),
                                  ctypes.POINTER(c_int)]),
    "clasfv_fill_workspace": (c_int, [_P, c_int, _P]),
    "clasfv_workspace_view": (c_int, [_P, _P, ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64)]),
    "clasfv_forward_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(PlanLaunch),
                                    ctypes.POINTER(c_int), c_int, ctypes.POINTER(PlanBuffer), ctypes.POINTER(c_int)]),
    "clasfv_plan_conv_info": (c_int, [c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                      ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "clasfv_conv_count": (c_int, [_P]),
    "clasfv_conv_info": (c_int, [_P, c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_char_p), ctypes.POINTER(c_int),
                                 ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                 ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "clasfv_run_conv": (c_int, [_P, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, c_int, c_int, c_int, _P, _P, c_int64,
                                ctypes.POINTER(c_char_p), _P]),
    "clasfv_run_decoder": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "clasfv_build_clips": (c_int, [_P, c_int, c_int, c_int, _P, c_int, c_int, _P, _P]),
    "clasfv_pass_labels": (c_int, [_P, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "clasfv_pass_labels_margin": (c_int, [_P, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "clasfv_logit_margin": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "clasfv_fuse_votes": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "clasfv_warp": (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int64, c_int64, _P, _P]),
    "clasfv_zeroone_workspace_bytes": (c_int64, []),
    "clasfv_zeroone_normalize": (c_int, [_P, c_int64, _P, _P]),
    "clasfv_warp_backward": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, c_int64, c_int64, _P, _P, _P]),
    "clasfv_preprocess_video": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "clasfv_track": (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int,
                             c_int, _P, _P]),
    "clasfv_lv_geometry": (c_int, [_P, c_int64, c_int, c_int, c_int, ctypes.c_double, ctypes.c_double, _P, _P, _P]),
    "clasfv_render_workspace_bytes": (c_int64, []),
    "clasfv_render_annotated": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, c_int64, _P, c_int, c_int, c_int, c_int,
                                        c_int, c_int, c_int, ctypes.c_double, _P, _P, _P]),
}

ABI_VERSION = 3  # CLASFV_ABI_VERSION of include/clasfv.h these signatures describe
FUSE_MAJORITY, FUSE_SIMPLE, FUSE_STAPLE, FUSE_ITKVOTING = 0, 1, 2, 3
FUSE_FORCE_GENERIC = 0x100
# CLASFV_FUSE_CLEAN, CLASFV_FUSE_CLEAN_HOLES(n), CLASFV_CLEAN_* (include/clasfv.h)
FUSE_CLEAN = 0x200
CLEAN_DEFAULT_HOLES, CLEAN_MAX_HOLES, CLEAN_MAX_PIXELS = 128, 32767, 53248


def fuse_clean_holes(n):
    """CLASFV_FUSE_CLEAN_HOLES(n): the hole threshold in bits 16..30 of a clasfv_fuse_votes method."""
    return n << 16


def clean_bits(holesize, name="holesize"):
    """CLASFV_FUSE_CLEAN with its hole threshold, for OR-ing into a method; ValueError unless ``holesize`` is
    an integer in 1..32767. Host arithmetic."""
    if isinstance(holesize, bool) or not isinstance(holesize, numbers.Integral) or not 1 <= holesize <= CLEAN_MAX_HOLES:
        raise ValueError(f"{name} {holesize!r} must be an integer in 1..{CLEAN_MAX_HOLES}")
    return FUSE_CLEAN | fuse_clean_holes(int(holesize))


def check_clean_frame(h, w, name):
    """ValueError for a frame the cleanup kernel cannot hold (CLASFV_CLEAN_MAX_PIXELS)."""
    if h * w > CLEAN_MAX_PIXELS:
        raise ValueError(f"{name}: cleanup takes frames of at most {CLEAN_MAX_PIXELS} pixels, got {h} x {w}")
# CLASFV_TRACK_* (include/clasfv.h)
TRACK_BILINEAR, TRACK_NEAREST = 0, 1
TRACK_FORCE_STEPS, TRACK_FORCE_LDS = 0x100, 0x200
TRACK_LDS_MAX_PIXELS, TRACK_LDS_AUTO_PIXELS = 20480, 2304
# CLASFV_LV_* (include/clasfv.h)
LV_NPUCKS, LV_STRIDE, LV_MAX_PIXELS = 10, 12, 162816
# CLASFV_VARIANT_* bits (include/clasfv.h)
VARIANTS = {"no_winograd": 1, "no_wino_patch": 2, "winot_reference": 4, "no_c8": 8, "no_stem_bf16": 16,
            "no_patch_bf16": 32, "no_decoder_bf16": 64, "winot_no_ts1": 128, "no_split_k": 256, "no_wino4": 512,
            "no_decoder_x3": 1024, "no_dma_x3": 2048, "no_stem_x3": 4096, "no_wino4w": 8192,
            "no_patch32": 16384, "no_proj_x3": 32768, "no_wino4r": 65536,
            "no_dma_buf": 262144, "w4r_cached_stores": 524288,
            "patch32_cached_stores": 4194304, "no_dma_w": 16777216, "no_twalk": 67108864}
# CLASFV_VARIANT_NO_DMA_X3_WIDE (a #define beside the enum): conv_dma_x3 never in its wide form; pass the bit itself
NO_DMA_X3_WIDE = 268435456
DTYPES = {"fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1}
_lib = None


def lib_path():
    return LIB_PATH


def load():
    """Load and return the ctypes library. A library whose embedded source hash differs from the
    sources on disk (older than them, or built from other ones) is rebuilt before it is loaded --
    never used stale; without hipcc that rebuild raises."""
    global _lib
    if _lib is not None:
        return _lib
    from . import build as B
    want = B.source_hash()
    have = B.library_hash()
    if have != want:
        import sys
        print(f"clasfv: {LIB_PATH} {'missing' if have is None and not os.path.exists(LIB_PATH) else 'stale'} "
              f"(library source hash {have}, sources {want}): rebuilding", file=sys.stderr)
        # not forced: build() re-checks the hash under its lock, so ranks that waited for another
        # rank's rebuild reuse it instead of compiling again
        B.build()
        if B.library_hash() != want:
            raise RuntimeError(f"{LIB_PATH}: rebuild did not produce a library of the current sources")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.clasfv_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH}: ABI version {lib.clasfv_version()}, expected {ABI_VERSION}: rebuild it "
                           f"(python -m clasfv_amd.build --force)")
    got = lib.clasfv_source_hash().decode()
    if got != B.HASH_MARK.decode() + want:
        raise RuntimeError(f"{LIB_PATH}: loaded library reports {got}, sources hash to {want}")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().clasfv_last_error()
        raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
    return rc


def stream_ptr(stream=None, device=None):
    """hipStream_t of ``stream``, else the current stream of ``device`` (a tensor's device: the
    stream the caller's work on that device is ordered on), else of the current device."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return ctypes.c_void_p(s.cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def on_gpu(t, name, device=None, dtype=None):
    """``t`` if it is a tensor on a GPU (on ``device`` and of ``dtype`` where given), else TypeError for
    anything that is no tensor and ValueError naming the argument: the C ABI takes raw device pointers and
    cannot tell what they point at, so this is the only place a host tensor or another dtype is caught.
    Host comparisons only: no device work, no synchronisation."""
    import torch
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch tensor on the GPU (the library reads its device pointer), not "
                        f"{type(t).__name__}")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} (the library reads its bytes as that type), not {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be on the GPU (the library reads its device pointer), not on {t.device}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} must be on {device}, not on {t.device}")
    return t


def byte_span(t):
    """[lo, hi) of the addresses a tensor's elements occupy (strides are not negative in torch); an empty
    tensor spans nothing."""
    if t.numel() == 0:
        return t.data_ptr(), t.data_ptr()
    last = sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()


def overlap(a, b):
    """Whether the byte spans of two tensors intersect (the same tensor included)."""
    (alo, ahi), (blo, bhi) = byte_span(a), byte_span(b)
    return alo < ahi and blo < bhi and alo < bhi and blo < ahi
