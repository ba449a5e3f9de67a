"""What every data-taking export of libclasfv.so may touch through each pointer it is given, and a proxy
that holds the calls of the Python surface against it.

The C ABI (include/clasfv.h) takes raw pointers and a few integers. A wrong pointer or length either faults
the GPU or returns plausible numbers computed from the wrong bytes; neither is a kernel bug, and no kernel
test can see it. Two parts, neither of which needs a GPU to import:

``FOOTPRINT``: one rule per data-taking export. A rule maps the call's arguments to one ``Range`` per pointer
argument: read or written, element size, whether NULL is allowed, the alignment the header demands and the
byte range [0, bytes) the call may touch from the pointer. The rules restate the header's text (layouts,
strides, counts), not the kernels. clasfv_run_conv and clasfv_run_decoder are left out on purpose: they are
diagnostics driven only by tests that band their tensors with guard elements and check them after every
launch; they are in ``EXEMPT`` with the handle and introspection functions, which take no device data.

``AuditedLib``: a proxy around the loaded ctypes library (``install`` monkeypatches ``_lib.load``, ``_lib._lib``
and ``_lib.ptr``). Before it forwards a call it checks

* integers: every Python integer lies in the range of the C type of its slot in ``_lib.SIGNATURES`` (ctypes
  drops the high bits of one that does not, silently: 2**32 + 5 arrives as 5);
* live allocation: every non-NULL device pointer lies in a live block of PyTorch's caching allocator and
  [ptr, ptr + bytes) ends inside what that block was asked for (``torch.cuda.memory_snapshot()``: an
  ``active_allocated`` block's address and ``requested_size``). Resolving against the allocator, not against
  a registry of tensors, covers the pointers the wrappers compute by hand (render.py's volume pointer,
  track's channel-pair offset). Where the snapshot lacks those fields the proxy falls back, for the rest of
  its life, to weak references to the tensors the test registered and those ``_lib.ptr`` saw (``resolver``
  names the mode, and the GPU test asserts the snapshot's). A pointer that resolves to nothing is a
  violation, and a host pointer resolves to nothing;
* alignment: to the element size, or to what the header demands;
* overlap: no written range overlaps another range of the same call (the header allows none on these exports;
  an in-place tensor is one read-write range);
* stream: the stream argument is the current stream of the device that owns the pointers.

A violation raises ``Violation`` in the test process before the real function is called, so an audited run
never launches a call that it found to be wrong.
"""
import ctypes
import operator
import weakref
from collections import Counter, namedtuple

CLIP = 32
LV_STRIDE = 12

# name: the parameter's; mode "r", "w" or "rw"; elem: bytes per element; bytes: the call may touch [0, bytes);
# nullable: NULL allowed; align: demanded alignment (None: the element size)
Range = namedtuple("Range", "name ptr mode elem bytes nullable align", defaults=(False, None))


class Violation(AssertionError):
    pass


def _addr(p):
    """Integer address of a ctypes pointer argument (None and NULL: 0)."""
    if p is None:
        return 0
    if isinstance(p, int):
        return p
    if isinstance(p, ctypes.c_void_p):
        return p.value or 0
    return ctypes.cast(p, ctypes.c_void_p).value or 0


def n_clips(t):
    """The header's clip count of a t-frame pass: round(t / 32), half to even."""
    return int(round(t / CLIP))


def _host_ints(p, n):
    return list(ctypes.cast(ctypes.c_void_p(_addr(p)), ctypes.POINTER(ctypes.c_int32))[:n])


# ---- the rules: f(lib, *args of the export) -> [Range] ------------------------------------------------------
def _forward(lib, h, x, N, T, H, W, seg, mot, stream):
    vox = N * T * H * W
    return [Range("x_dev", x, "r", 4, 3 * vox * 4), Range("seg_dev", seg, "w", 4, 2 * vox * 4),
            Range("motion_dev", mot, "w", 4, 4 * vox * 4)]


def _build_clips(lib, video, T, H, W, table, n, interpolate, clips, stream):
    return [Range("video_dev", video, "r", 4, 3 * T * H * W * 4), Range("table_dev", table, "r", 4, 2 * n * 4),
            Range("clips_dev", clips, "w", 4, n * 3 * CLIP * H * W * 4)]


def _pass_labels(planes):
    def rule(lib, logits, K, clip0, T, step, H, W, interpolate, labels, stream):
        first = _host_ints(clip0, K)   # a host array of K ints
        clips = max(c + n_clips(T - k * step) for k, c in enumerate(first))
        return [Range("logits_dev", logits, "r", 4, clips * planes * CLIP * H * W * 4),
                Range("labels_dev", labels, "w", 1, K * T * H * W)]
    return rule


def _logit_margin(lib, logits, n, H, W, margin, stream):
    return [Range("logits_dev", logits, "r", 4, n * 2 * CLIP * H * W * 4),
            Range("margin_dev", margin, "w", 4, n * CLIP * H * W * 4)]


def _fuse_votes(lib, labels, K, T, step, H, W, method, fused, stream):
    return [Range("labels_dev", labels, "r", 1, K * T * H * W),
            Range("fused_dev", fused, "w", 1, (T - (step - 1)) * H * W)]


def _motion_bytes(N, H, W, m_sn, m_sc, extra=0):
    return ((N - 1) * m_sn + m_sc + extra + H * W) * 4


def _warp(lib, img, N, C, H, W, motion, m_sn, m_sc, out, stream):
    return [Range("img_dev", img, "r", 4, N * C * H * W * 4),
            Range("motion_dev", motion, "r", 4, _motion_bytes(N, H, W, m_sn, m_sc)),
            Range("out_dev", out, "w", 4, N * C * H * W * 4)]


def _warp_backward(lib, gout, img, N, C, H, W, motion, m_sn, m_sc, gimg, gmot, stream):
    return [Range("grad_out_dev", gout, "r", 4, N * C * H * W * 4), Range("img_dev", img, "r", 4, N * C * H * W * 4),
            Range("motion_dev", motion, "r", 4, _motion_bytes(N, H, W, m_sn, m_sc)),
            Range("grad_img_dev", gimg, "rw", 4, N * C * H * W * 4, True),    # accumulated into
            Range("grad_motion_dev", gmot, "w", 4, N * 2 * H * W * 4, True)]


def _track(lib, img, N, C, H, W, motion, m_sn, m_sc, m_st, T, t0, t_step, P, mode, out, stream):
    return [Range("img_dev", img, "r", 4, N * C * H * W * 4),
            Range("motion_dev", motion, "r", 4, _motion_bytes(N, H, W, m_sn, m_sc, (T - 1) * m_st)),
            Range("out_dev", out, "w", 4, P * N * C * H * W * 4)]


def _zeroone(lib, video, n_per_channel, workspace, stream):
    return [Range("video_dev", video, "rw", 4, 3 * n_per_channel * 4),
            Range("workspace_dev", workspace, "rw", 4, int(lib.clasfv_zeroone_workspace_bytes()))]


def _preprocess(lib, frames, T, Hs, Ws, H, W, out, stream):
    return [Range("frames_dev", frames, "r", 1, T * Hs * Ws * 3), Range("out_dev", out, "w", 4, 3 * T * H * W * 4)]


def _lv_geometry(lib, masks, F, H, W, label, sy, sx, area, geom, stream):
    return [Range("masks_dev", masks, "r", 1, F * H * W), Range("area_dev", area, "w", 4, F * 4),
            Range("geom_dev", geom, "w", 8, F * LV_STRIDE * 8, False, 8)]


def _render(lib, video, masks, truth, T, H, W, volume, vstride, title, first, count, Hp, Wo, Ht, Hs, label, thickness,
            workspace, out, stream):
    return [Range("video_dev", video, "r", 4, 3 * T * H * W * 4), Range("masks_dev", masks, "r", 1, T * H * W),
            Range("truth_dev", truth, "r", 1, T * H * W, True),
            Range("volume_dev", volume, "r", 8, ((T - 1) * vstride + 1) * 8, False, 8),
            Range("title_dev", title, "r", 1, Ht * Wo * 3, True),
            Range("workspace_dev", workspace, "rw", 8, int(lib.clasfv_render_workspace_bytes()), False, 8),
            Range("out_dev", out, "w", 1, count * (Hp + Ht + Hs) * Wo * 3)]


FOOTPRINT = {
    "clasfv_forward": _forward, "clasfv_build_clips": _build_clips,
    "clasfv_pass_labels": _pass_labels(2), "clasfv_pass_labels_margin": _pass_labels(1),
    "clasfv_logit_margin": _logit_margin, "clasfv_fuse_votes": _fuse_votes,
    "clasfv_warp": _warp, "clasfv_warp_backward": _warp_backward, "clasfv_track": _track,
    "clasfv_zeroone_normalize": _zeroone, "clasfv_preprocess_video": _preprocess,
    "clasfv_lv_geometry": _lv_geometry, "clasfv_render_annotated": _render,
}

# Exports with a pointer or stream argument that have no rule, and why. No data-taking export is here.
EXEMPT = {
    # the handle: host objects, host arrays and strings only
    "clasfv_create": "handle", "clasfv_destroy": "handle", "clasfv_load_param": "handle (host data)",
    "clasfv_finalize": "handle", "clasfv_set_compute_dtype": "handle", "clasfv_get_compute_dtype": "handle",
    "clasfv_set_kernel_variants": "handle", "clasfv_get_kernel_variants": "handle",
    # introspection: the handle and host output arrays
    "clasfv_param_count": "introspection", "clasfv_param_info": "introspection",
    "clasfv_workspace_bytes": "introspection", "clasfv_conv_count": "introspection", "clasfv_conv_info": "introspection",
    "clasfv_plan_conv_info": "introspection", "clasfv_forward_plan": "introspection",
    "clasfv_set_kernel_timing": "introspection", "clasfv_kernel_timing": "introspection",
    "clasfv_set_launch_log": "introspection", "clasfv_launch_log": "introspection",
    "clasfv_workspace_view": "introspection",
    # diagnostics: the library's own arena, and the single-layer entry points whose tests band their tensors
    "clasfv_fill_workspace": "diagnostics", "clasfv_run_conv": "diagnostics", "clasfv_run_decoder": "diagnostics",
}


def takes_pointer_or_stream(argtypes):
    return any(a is ctypes.c_void_p or (isinstance(a, type) and issubclass(a, ctypes._Pointer)) or a is ctypes.c_char_p
               for a in argtypes)


_INT_RANGES = {ctypes.c_int: (-2 ** 31, 2 ** 31 - 1), ctypes.c_int64: (-2 ** 63, 2 ** 63 - 1)}


def integer_problems(name, argtypes, args):
    bad = []
    for i, (tp, v) in enumerate(zip(argtypes, args)):
        if tp not in _INT_RANGES:
            continue
        try:
            v = operator.index(v)
        except TypeError:
            bad.append(f"{name}: argument {i} = {v!r} is no integer for its {tp.__name__}")
            continue
        lo, hi = _INT_RANGES[tp]
        if not lo <= v <= hi:
            bad.append(f"{name}: argument {i} = {v} does not fit its {tp.__name__} (ctypes would pass {tp(v).value})")
    return bad


def overlap_problems(name, ranges):
    live = [r for r in ranges if _addr(r.ptr) and r.bytes > 0]
    bad = []
    for i, a in enumerate(live):
        for b in live[i + 1:]:
            if "w" not in a.mode and "w" not in b.mode:
                continue
            alo, blo = _addr(a.ptr), _addr(b.ptr)
            if alo < blo + b.bytes and blo < alo + a.bytes:
                bad.append(f"{name}: {a.name} [{alo:#x}, +{a.bytes}) overlaps {b.name} [{blo:#x}, +{b.bytes})")
    return bad


class AuditedLib:
    """Proxy of the ctypes library: ``lib.clasfv_x(...)`` checks the call, then forwards it. ``calls`` counts the
    exports reached; ``blocks`` may replace the allocator snapshot (a list of (address, bytes, device) live
    blocks) for host-side tests of the audit itself."""

    def __init__(self, real, signatures, blocks=None, current_stream=None):
        self._real, self._sig = real, signatures
        self._blocks, self._current_stream = blocks, current_stream
        self.calls = Counter()
        self.tensors = {}                 # id -> weak reference: the fallback registry; dead tensors drop out
        self.use_registry = False         # set, for good, when the snapshot lacks a field

    @property
    def resolver(self):
        """What resolves pointers: "given blocks" (host tests), "allocator snapshot" or "tensor registry"."""
        return "given blocks" if self._blocks is not None else "tensor registry" if self.use_registry else \
            "allocator snapshot"

    def register(self, *tensors):
        """Tensors whose pointers reach the library without passing _lib.ptr (the registry's only other source)."""
        for t in tensors:   # by identity: tensors compare elementwise, so no set of them
            key = id(t)
            self.tensors[key] = weakref.ref(t, lambda _, key=key: self.tensors.pop(key, None))
        return tensors[0] if len(tensors) == 1 else tensors

    # ---- pointer resolution ------------------------------------------------------------------------------
    def live_blocks(self):
        """[(address, bytes asked for, device index)] of every live allocation."""
        if self._blocks is not None:
            return list(self._blocks)
        import torch
        out = []
        if not self.use_registry:
            for seg in torch.cuda.memory_snapshot():
                at = seg.get("address")
                for b in seg.get("blocks", ()):
                    if at is None or "size" not in b or "requested_size" not in b or "state" not in b:
                        self.use_registry = True
                        break
                    addr = b.get("address", at)
                    at = addr + b["size"]
                    if b["state"] == "active_allocated":
                        out.append((addr, b["requested_size"], seg.get("device", 0)))
                if self.use_registry:
                    break
        if self.use_registry:
            out = []
            for ref in list(self.tensors.values()):
                t = ref()
                if t is not None and t.is_cuda:
                    st = t.untyped_storage()
                    out.append((st.data_ptr(), st.nbytes(), t.device.index))
        return out

    def resolve(self, addr, nbytes, blocks):
        """(device, None) of the live block holding [addr, addr + nbytes), or (None, why not)."""
        for lo, size, dev in blocks:
            if lo <= addr < lo + size:
                if addr + nbytes <= lo + size:
                    return dev, None
                return None, f"runs {addr + nbytes - lo - size} bytes past its allocation of {size} bytes"
        return None, "lies in no live device allocation (a host pointer, or freed memory)"

    def current_stream(self, dev):
        if self._current_stream is not None:
            return self._current_stream
        import torch
        return torch.cuda.current_stream(dev).cuda_stream or 0

    # ---- the checks --------------------------------------------------------------------------------------
    def problems(self, name, args):
        res, argtypes = self._sig[name]
        bad = integer_problems(name, argtypes, args)
        if len(args) != len(argtypes):
            bad.append(f"{name}: {len(args)} arguments for {len(argtypes)} parameters")
        if bad or name not in FOOTPRINT:
            return bad
        ranges = FOOTPRINT[name](self._real, *args)
        blocks = self.live_blocks()
        devices = set()
        for r in ranges:
            addr = _addr(r.ptr)
            if addr == 0:
                if not r.nullable:
                    bad.append(f"{name}: {r.name} is NULL")
                continue
            if r.bytes < 0:
                bad.append(f"{name}: {r.name} has a negative extent {r.bytes}")
                continue
            align = r.align or r.elem
            if addr % align:
                bad.append(f"{name}: {r.name} = {addr:#x} is not aligned to {align} bytes")
            dev, why = self.resolve(addr, r.bytes, blocks)
            if why:
                bad.append(f"{name}: {r.name} = {addr:#x} (+{r.bytes} bytes, {r.mode}) {why}")
            else:
                devices.add(dev)
        bad += overlap_problems(name, ranges)
        if len(devices) > 1:
            bad.append(f"{name}: pointers on several devices {sorted(devices)}")
        elif len(devices) == 1:
            want, got = self.current_stream(devices.pop()), _addr(args[-1])
            if got != want:
                bad.append(f"{name}: stream {got:#x} is not the current stream {want:#x} of the pointers' device")
        return bad

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._sig:
            return fn

        def audited(*args):
            bad = self.problems(name, args)
            if bad:
                raise Violation("; ".join(bad))
            self.calls[name] += 1
            return fn(*args)
        audited.__name__ = name
        return audited


def install(monkeypatch, lib_module, real=None):
    """Put an AuditedLib where the package finds its library; returns it. ``lib_module``: the package's _lib."""
    real = lib_module.load() if real is None else real
    audited = AuditedLib(real, lib_module.SIGNATURES)
    real_ptr = lib_module.ptr

    def ptr(t):
        audited.register(t)
        return real_ptr(t)
    monkeypatch.setattr(lib_module, "load", lambda: audited)
    monkeypatch.setattr(lib_module, "_lib", audited)
    monkeypatch.setattr(lib_module, "ptr", ptr)
    return audited
