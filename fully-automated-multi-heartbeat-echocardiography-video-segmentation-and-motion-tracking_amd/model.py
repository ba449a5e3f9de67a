"""Drop-in ``R2plus1D_18_MotionNet`` backed by the HIP engine (libclasfv.so).

Mirrors src/model/R2plus1D_18_MotionNet.py:10-71: ``forward(x) -> (segmentation_logits, motion)``
with x (N,3,T,H,W) float32, seg (N,2,T,H,W) and motion (N,4,T,H,W) = tanh(...). The state dict has
the reference's 242 keys; ``load_state_dict`` accepts the ``module.``-prefixed keys that
``nn.DataParallel`` checkpoints carry (motion_segment.py:69-72).

Differences, all deliberate:
* ``pretrained=True`` cannot download Kinetics weights offline; the network starts from seeded
  synthetic weights (``weights="random"``: weights.synthetic_state_dict; ``weights="echo"``: the
  recipe whose masks follow the synthetic video's LV, weights.echo_state_dict) and a checkpoint is
  expected to be loaded.
* Inference only: forward runs under no autograd (the reference builds graphs it never uses,
  src/fuse_utils.py:59).
* Any H, W multiple of 16 and T multiple of 8 is accepted (the reference's concat needs the same).
"""
import ctypes
import warnings
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from . import _lib
from .arch import strip_module_prefix
from .weights import DEFAULT_SEED, recipe_state_dict


def variant_flags(names):
    """CLASFV_VARIANT_* bits of variant names (an int passes through, alone or among the names)."""
    if isinstance(names, int):
        return names
    flags = 0
    for n in names:
        if isinstance(n, int):
            flags |= n
            continue
        if n not in _lib.VARIANTS:
            raise ValueError(f"unknown kernel variant {n!r}: {sorted(_lib.VARIANTS)}")
        flags |= _lib.VARIANTS[n]
    return flags


def forward_plan(n, t, h, w, dtype="fp32", variants=()):
    """clasfv_forward_plan: what a forward of n clips of (t, h, w) issues on an engine of `dtype` and `variants`
    (names or bits), as {"launches": [...], "buffers": [...]}; host arithmetic, needs no GPU. A launch is a
    dict of clasfv_plan_launch_t's fields with "kind" and each range's "role" as their names (_lib.PLAN_KINDS,
    _lib.PLAN_ROLES) and "ranges" a list of {"buffer", "role", "write", "offset", "bytes"}; a buffer row a dict
    of clasfv_plan_buffer_t's."""
    lib = _lib.load()
    args = (n, t, h, w, _lib.DTYPES[dtype], variant_flags(variants))
    nl, nbuf = ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.clasfv_forward_plan(*args, 0, None, ctypes.byref(nl), 0, None, ctypes.byref(nbuf)), "clasfv_forward_plan")
    launches, buffers = (_lib.PlanLaunch * nl.value)(), (_lib.PlanBuffer * nbuf.value)()
    _lib.check(lib.clasfv_forward_plan(*args, nl.value, launches, ctypes.byref(nl), nbuf.value, buffers,
                                       ctypes.byref(nbuf)), "clasfv_forward_plan")
    scalars = ("sub_batch", "stream", "conv", "split_asked", "split_granted", "x_c8", "y_c8", "relu", "has_res",
               "x_elem", "y_elem")
    out = []
    for l in launches:
        d = {k: int(getattr(l, k)) for k in scalars}
        d["kind"] = _lib.PLAN_KINDS[l.kind]
        d["kernel"] = l.kernel.decode()
        d["ranges"] = [{"buffer": int(r.buffer), "role": _lib.PLAN_ROLES[r.role], "write": bool(r.write),
                        "offset": int(r.offset), "bytes": int(r.bytes)} for r in l.range[:l.n_ranges]]
        out.append(d)
    rows = [{"sub_batch": int(b.sub_batch), "clips": int(b.clips), "id": int(b.id), "name": b.name.decode(),
             "offset": int(b.offset), "bytes": int(b.bytes), "total": int(b.total)} for b in buffers]
    return {"launches": out, "buffers": rows}


def plan_conv_table(dtype="fp32"):
    """Engine.conv_table()'s channels, kernel, stride, padding and dtypes for an engine of `dtype`, without a
    handle (clasfv_plan_conv_info): one dict per conv, the backbone in execution order, then P01, P2, P3, P4."""
    lib = _lib.load()
    out = []
    din, dout = ctypes.c_int(), ctypes.c_int()
    ch, k, s, p = (ctypes.c_int * 5)(), (ctypes.c_int * 3)(), (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    while lib.clasfv_plan_conv_info(_lib.DTYPES[dtype], len(out), ch, k, s, p, ctypes.byref(din), ctypes.byref(dout)) == 0:
        out.append({"index": len(out), "cin": ch[0], "cout": ch[1], "cin_p": ch[2], "cout_p": ch[3], "cin2": ch[4],
                    "kernel": tuple(k), "stride": tuple(s), "padding": tuple(p),
                    "in_dtype": torch.bfloat16 if din.value == 1 else torch.float32,
                    "out_dtype": torch.bfloat16 if dout.value == 1 else torch.float32})
    return out


class Engine:
    """Owns one clasfv handle (weights + workspace) on one HIP device."""

    def __init__(self, device=None, dtype="fp32"):
        if not torch.cuda.is_available():
            raise RuntimeError("CLAS-FV engine requires a HIP (ROCm) GPU; none is visible")
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   torch.device(device).index or 0)
        h = ctypes.c_void_p()
        _lib.check(self.lib.clasfv_create(self.device.index, ctypes.byref(h)), "clasfv_create")
        self.h = h
        self.set_dtype(dtype)

    def set_dtype(self, dtype):
        """'fp32' (default, reference precision) or 'bf16' (BASELINE config[4]); re-load weights after."""
        if dtype not in _lib.DTYPES:
            raise ValueError(f"dtype must be one of {sorted(_lib.DTYPES)}")
        _lib.check(self.lib.clasfv_set_compute_dtype(self.h, _lib.DTYPES[dtype]), "clasfv_set_compute_dtype")
        self.dtype = "bf16" if _lib.DTYPES[dtype] == 1 else "fp32"

    def set_variants(self, *names):
        """Kernel variants for A/B tests (CLASFV_VARIANT_*; e.g. "no_winograd"); no names = the
        product kernels. Returns the previous names. Call load() afterwards if no_winograd changed."""
        flags = variant_flags(names)
        old = self.lib.clasfv_get_kernel_variants(self.h)
        _lib.check(self.lib.clasfv_set_kernel_variants(self.h, flags), "clasfv_set_kernel_variants")
        return tuple(n for n, b in _lib.VARIANTS.items() if old & b)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.clasfv_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def param_table(self):
        out = []
        name = ctypes.c_char_p()
        nd = ctypes.c_int()
        dims = (ctypes.c_int64 * 5)()
        for i in range(self.lib.clasfv_param_count(self.h)):
            _lib.check(self.lib.clasfv_param_info(self.h, i, ctypes.byref(name), ctypes.byref(nd), dims), "param_info")
            out.append((name.value.decode(), tuple(int(dims[d]) for d in range(nd.value))))
        return out

    def load(self, state):
        for k, v in state.items():
            a = np.ascontiguousarray(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v), dtype=np.float32)
            _lib.check(self.lib.clasfv_load_param(self.h, k.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size),
                       f"load {k}")
        _lib.check(self.lib.clasfv_finalize(self.h), "clasfv_finalize")

    def forward(self, x, seg, mot, stream=None):
        """x (n,3,t,h,w) -> seg (n,2,t,h,w) logits and mot (n,4,t,h,w), written into the caller's buffers:
        all three contiguous float32 tensors on the engine's device, seg and mot overlapping neither each
        other nor x (ValueError otherwise; nothing is converted, the library reads and writes their bytes)."""
        for name, a in (("x", x), ("seg", seg), ("mot", mot)):
            _lib.on_gpu(a, name, self.device, torch.float32)
        if x.dim() != 5 or x.shape[1] != 3 or not x.is_contiguous():
            raise ValueError(f"x: a contiguous (n,3,t,h,w) tensor expected, got {tuple(x.shape)} with strides {x.stride()}")
        n, c, t, hh, ww = x.shape
        for name, a, ch in (("seg", seg, 2), ("mot", mot, 4)):
            if tuple(a.shape) != (n, ch, t, hh, ww) or not a.is_contiguous():
                raise ValueError(f"{name}: a contiguous {(n, ch, t, hh, ww)} tensor expected for x {tuple(x.shape)}, got "
                                 f"{tuple(a.shape)} with strides {a.stride()}")
        for (na, a), (nb, b) in ((("seg", seg), ("mot", mot)), (("seg", seg), ("x", x)), (("mot", mot), ("x", x))):
            if _lib.overlap(a, b):
                raise ValueError(f"{na} overlaps {nb}: the forward writes its outputs while it reads its input")
        _lib.check(self.lib.clasfv_forward(self.h, _lib.ptr(x), n, t, hh, ww, _lib.ptr(seg), _lib.ptr(mot),
                                           _lib.stream_ptr(stream, self.device)), "clasfv_forward")

    # ---- diagnostics: one layer alone (tests) ---------------------------------------------------------
    def conv_table(self):
        """One dict per conv of clasfv_conv_info (backbone in execution order, then P01, P2, P3, P4)."""
        out = []
        pre, bn = ctypes.c_char_p(), ctypes.c_char_p()
        tap, din, dout = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        ch, k, s, p = (ctypes.c_int * 5)(), (ctypes.c_int * 3)(), (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
        for i in range(self.lib.clasfv_conv_count(self.h)):
            _lib.check(self.lib.clasfv_conv_info(self.h, i, ctypes.byref(pre), ctypes.byref(bn), ctypes.byref(tap), ch, k, s,
                                                 p, ctypes.byref(din), ctypes.byref(dout)), "clasfv_conv_info")
            out.append({"index": i, "prefix": pre.value.decode(), "bn": bn.value.decode(), "tap": tap.value,
                        "cin": ch[0], "cout": ch[1], "cin_p": ch[2], "cout_p": ch[3], "cin2": ch[4],
                        "kernel": tuple(k), "stride": tuple(s), "padding": tuple(p),
                        "in_dtype": torch.bfloat16 if din.value == 1 else torch.float32,
                        "out_dtype": torch.bfloat16 if dout.value == 1 else torch.float32})
        return out

    def run_conv(self, i, x, nthw, y, x2=None, res=None, relu=True, x_c8=False, y_c8=False, scratch=None, stream=None):
        """clasfv_run_conv on device tensors in the engine's layouts; returns the kernel's name."""
        name = ctypes.c_char_p()
        n, t, hh, ww = nthw
        opt = lambda a: _lib.ptr(a) if a is not None else None
        _lib.check(self.lib.clasfv_run_conv(self.h, i, _lib.ptr(x), n, t, hh, ww, opt(x2), opt(res), int(bool(relu)),
                                            int(bool(x_c8)), int(bool(y_c8)), _lib.ptr(y), opt(scratch),
                                            scratch.numel() * scratch.element_size() if scratch is not None else 0,
                                            ctypes.byref(name), _lib.stream_ptr(stream, self.device)), "clasfv_run_conv")
        return name.value.decode()

    def run_decoder(self, taps, nthw, seg, mot, stream=None):
        """clasfv_run_decoder over the four projected taps (channels-last fp32, 64 channels)."""
        n, t, hh, ww = nthw
        _lib.check(self.lib.clasfv_run_decoder(self.h, *[_lib.ptr(a) for a in taps], n, t, hh, ww, _lib.ptr(seg),
                                               _lib.ptr(mot), _lib.stream_ptr(stream, self.device)), "clasfv_run_decoder")

    def set_launch_log(self, enable=True):
        """Record every kernel launch of later forward / run_conv / run_decoder calls (clasfv_launch_log)."""
        _lib.check(self.lib.clasfv_set_launch_log(self.h, 1 if enable else 0), "clasfv_set_launch_log")

    def launch_log(self, cap=4096):
        """[(label, grid, passes, conv)] of the launches since the last call, in order (then cleared).
        label: the instantiation as the compiler spells it, e.g. "conv_winot5<4, 4, 2>" (an opaque key; the
        part before "<" is the kernel's name); passes: work items per wave or block of a capped grid, else 1;
        conv: clasfv_conv_info's index, -1 for pack_input_kernel and the decoder."""
        labels = (ctypes.c_char_p * cap)()
        grids = (ctypes.c_int64 * cap)()
        passes = (ctypes.c_int * cap)()
        convs = (ctypes.c_int * cap)()
        n = self.lib.clasfv_launch_log(self.h, cap, labels, grids, passes, convs)
        if n < 0:
            _lib.check(n, "clasfv_launch_log")
        return [(labels[i].decode(), int(grids[i]), int(passes[i]), int(convs[i])) for i in range(n)]

    def set_kernel_timing(self, enable=True):
        """Per-kernel HIP-event timing of every later forward (see clasfv_kernel_timing)."""
        _lib.check(self.lib.clasfv_set_kernel_timing(self.h, 1 if enable else 0), "clasfv_set_kernel_timing")

    def kernel_timing(self, cap=16):
        """{kernel: {"launches", "ms", "gflop", "xgflop"}} over the forwards since the last call (then
        cleared). gflop: algorithmic (direct-conv MACs x 2); xgflop: MFMA work actually issued."""
        names = (ctypes.c_char_p * cap)()
        launches = (ctypes.c_int * cap)()
        ms = (ctypes.c_double * cap)()
        gf = (ctypes.c_double * cap)()
        xg = (ctypes.c_double * cap)()
        n = self.lib.clasfv_kernel_timing(self.h, cap, names, launches, ms, gf, xg)
        if n < 0:
            _lib.check(n, "clasfv_kernel_timing")
        return {names[i].decode(): {"launches": int(launches[i]), "ms": float(ms[i]), "gflop": float(gf[i]),
                                    "xgflop": float(xg[i])} for i in range(n)}

    def max_clips(self, t, h, w):
        """The largest batch of (t, h, w) clips one pass of the network takes with this engine's dtype and
        variants (clasfv_max_clips); forward() runs a larger one as sub-batches of that many clips."""
        n = self.lib.clasfv_max_clips(t, h, w, _lib.DTYPES[self.dtype], self.lib.clasfv_get_kernel_variants(self.h))
        if n < 0:
            _lib.check(n, "clasfv_max_clips")
        return n

    def workspace_bytes(self):
        return int(self.lib.clasfv_workspace_bytes(self.h))

    def fill_workspace(self, byte, stream=None):
        """Fill the whole workspace arena of `stream`'s context with `byte` (clasfv_fill_workspace; tests)."""
        _lib.check(self.lib.clasfv_fill_workspace(self.h, int(byte), _lib.stream_ptr(stream, self.device)),
                   "clasfv_fill_workspace")

    def workspace_view(self, stream=None):
        """(device address, bytes) of the arena of `stream`'s context (clasfv_workspace_view; tests)."""
        base, size = ctypes.c_void_p(), ctypes.c_int64()
        _lib.check(self.lib.clasfv_workspace_view(self.h, _lib.stream_ptr(stream, self.device), ctypes.byref(base),
                                                  ctypes.byref(size)), "clasfv_workspace_view")
        return int(base.value), int(size.value)

    def forward_plan(self, n, t, h, w):
        """forward_plan() of n clips of (t, h, w) for this engine's dtype and variants."""
        return forward_plan(n, t, h, w, self.dtype, self.lib.clasfv_get_kernel_variants(self.h))


class R2plus1D_18_MotionNet(nn.Module):
    """HIP-backed drop-in for the reference model (inference)."""

    def __init__(self, pretrained=True, output_channels=4, device=None, seed=DEFAULT_SEED, dtype="fp32",
                 weights="random"):
        super().__init__()
        if output_channels != 4:
            raise ValueError("the motion head has 4 channels [fwd x, fwd y, bwd x, bwd y]")
        if pretrained:
            warnings.warn("pretrained=True: Kinetics weights cannot be downloaded offline; using seeded synthetic "
                          "weights (load a checkpoint with load_state_dict)", stacklevel=2)
        self.engine = Engine(device, dtype)
        self._state = OrderedDict()
        self._params = None
        self._load(recipe_state_dict(weights, seed))

    def set_kernel_variants(self, *names):
        """A/B-test kernel variants (see Engine.set_variants); weights are re-uploaded so the
        choice of Winograd or direct weight images follows. Returns the previous variant names."""
        old = self.engine.set_variants(*names)
        self.engine.load(self._state)
        return old

    def set_compute_dtype(self, dtype):
        """Switch the encoder between exact fp32 and bf16 (fp32 accumulation) and re-upload weights."""
        self.engine.set_dtype(dtype)
        self.engine.load(self._state)
        return self

    # ---- state dict ------------------------------------------------------------------------------
    def _load(self, sd):
        table = self.engine.param_table()
        state = OrderedDict()
        for name, shape in table:
            if name not in sd:
                raise KeyError(f"missing key in state_dict: {name}")
            v = sd[name]
            t = v.detach().cpu() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))
            if tuple(t.shape) != shape:
                raise RuntimeError(f"size mismatch for {name}: {tuple(t.shape)} vs {shape}")
            state[name] = t.clone()
        self.engine.load(state)
        self._state = state
        self._params = None

    def load_state_dict(self, state_dict, strict=True):
        sd = OrderedDict((strip_module_prefix(k), v) for k, v in state_dict.items())
        expected = {n for n, _ in self.engine.param_table()}
        unexpected = [k for k in sd if k not in expected]
        missing = [k for k in expected if k not in sd]
        if strict and (unexpected or missing):
            raise RuntimeError(f"Error(s) in loading state_dict: missing={missing[:5]} unexpected={unexpected[:5]}")
        merged = OrderedDict(self._state)
        merged.update({k: v for k, v in sd.items() if k in expected})
        self._load(merged)
        return nn.modules.module._IncompatibleKeys(missing, unexpected)

    def state_dict(self, *args, **kwargs):
        return OrderedDict((k, v.clone()) for k, v in self._state.items())

    def parameters(self, recurse=True):
        if self._params is None:
            self._params = [nn.Parameter(v.float(), requires_grad=True) for k, v in self._state.items()
                            if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
        return iter(self._params)

    # ---- forward ---------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x):
        x = torch.as_tensor(x)
        if x.dim() != 5 or x.shape[1] != 3:
            raise ValueError(f"expected (N,3,T,H,W), got {tuple(x.shape)}")
        x = x.to(self.engine.device, torch.float32).contiguous()
        n, _, t, h, w = x.shape
        seg = torch.empty((n, 2, t, h, w), device=x.device, dtype=torch.float32)
        mot = torch.empty((n, 4, t, h, w), device=x.device, dtype=torch.float32)
        self.engine.forward(x, seg, mot)
        return seg, mot
