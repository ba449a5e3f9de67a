"""The launch plan is what runs: clasfv_forward_plan against a real forward's arena, launch log and sizes.

tests/test_plan_host.py audits the plan on the host; here the plan is tied to the kernels. Per case (the four
shapes of tests/test_engine_state_gpu.py with the product kernels, and every single variant at the ragged one,
both dtypes):

 a. a fresh handle's arena after its first forward has the plan's size;
 b. the launch log, in issue order with the side stream's launches where they were issued, is the plan's
    sequence of (conv, kernel), the split sums exactly where the plan grants a split;
 c. after a fill with 0xFF and one forward, every byte outside the plan's write ranges is still 0xFF (the
    slack between buffers, the unused tails, buffers the shape leaves partly unused), no element inside a
    range that holds activations or partial sums is all ones (nobody wrote it: outputs are finite and padded
    channels are +0), and the outputs are finite and bit-equal to the same forward over an arena of zeros:
    the in-situ counterpart of the isolated tests' guard bands, on the forward's own unguarded neighbours;
 d. clasfv_workspace_view refuses a null handle and a stream without a context.
"""
import ctypes

import numpy as np
import pytest
import torch

from clasfv_amd import _lib
from oracle import layer_ref as LR
from tests import plan_audit as PA
from tests import test_layers_gpu as TL

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "bf16")
SMALL, RAGGED, FIVE, CLIP = (1, 8, 16, 32), (2, 16, 64, 48), (3, 24, 80, 112), (1, 32, 112, 112)
SHAPES = (SMALL, RAGGED, FIVE, CLIP)


def shape_id(s):
    return "x".join(map(str, s))


def new_model(dtype):
    from clasfv_amd.model import R2plus1D_18_MotionNet
    return R2plus1D_18_MotionNet(pretrained=False, dtype=dtype)


def clip(shape, device):
    n, t, h, w = shape
    rng = np.random.default_rng(sum(shape) + 11)
    return torch.from_numpy(rng.uniform(0, 1, (n, 3, t, h, w)).astype(np.float32)).to(device)


def forward(model, x):
    def run():
        out = model(x)
        torch.cuda.synchronize()
        return out
    return TL.on_device(run)


class DeviceBytes:
    """Device memory the library owns, as the array interface torch.as_tensor takes (no copy)."""

    def __init__(self, address, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (address, False), "version": 2}


def arena_snapshot(eng):
    """A copy of the whole arena of the current stream's context, read through clasfv_workspace_view."""
    base, size = eng.workspace_view()
    torch.cuda.synchronize()
    snap = torch.as_tensor(DeviceBytes(base, size), device=eng.device).clone()
    torch.cuda.synchronize()
    assert snap.dtype == torch.uint8 and snap.numel() == size
    return snap


def log_sequence(log):
    return [(conv, TL.REPORTED_AS.get(TL.label_kernel(label), TL.label_kernel(label))) for label, _, _, conv in log]


def plan_sequence(plan):
    return [(l["conv"], l["kernel"]) for l in plan["launches"] if l["kind"] not in PA.MARKERS]


def check_case(model, shape, fresh):
    eng = model.engine
    n, t, h, w = shape
    plan = eng.forward_plan(n, t, h, w)
    assert PA.audit(plan) == [] and PA.check_split_sums(plan) == []
    assert PA.check_footprints(plan, eng.conv_table(), [n], t, h, w, LR.out_dim, LR.tap_shapes) == []
    total = plan["buffers"][0]["total"]
    x = clip(shape, eng.device)
    if fresh:
        assert eng.workspace_bytes() == 0
    eng.set_launch_log(True)
    try:
        first = forward(model, x)
        log = eng.launch_log()
    finally:
        eng.set_launch_log(False)
    # a. sizes
    base, size = eng.workspace_view()
    assert base != 0
    if fresh:
        assert eng.workspace_bytes() == size == total, (eng.workspace_bytes(), size, total)
    else:
        assert size >= total
    # b. sequences
    assert log_sequence(log) == plan_sequence(plan)
    sums = [conv for conv, k in log_sequence(log) if k == "split_sum_kernel"]
    assert sums == [l["conv"] for l in plan["launches"] if l["kind"] == "conv" and l["split_granted"] > 1]
    # c. writes land exactly where the plan says
    eng.fill_workspace(0xFF)
    torch.cuda.synchronize()
    dirty = forward(model, x)
    snap = arena_snapshot(eng)
    written = PA.written_elements(plan)
    holes = PA.uncovered(0, size, PA.merged((a, b) for a, b, _ in written))
    if eng.dtype == "bf16":  # 2-byte activations in buffers sized for 4: half of each is never written
        assert sum(b - a for a, b in holes) > size // 4
    for a, b in holes:
        bad = (snap[a:b] != 0xFF).nonzero()
        assert bad.numel() == 0, f"byte {a + int(bad[0])} of the arena, outside every write range of the plan, was written"
    checked = 0
    for a, b, es in written:
        if es is None:  # the decoder's index table
            continue
        assert a % es == 0 and (b - a) % es == 0
        bits = snap[a:b].view(torch.int16 if es == 2 else torch.int32)
        unset = (bits == -1).nonzero()
        assert unset.numel() == 0, (f"the {es}-byte element at arena byte {a + es * int(unset[0])}, inside a write range "
                                    f"of the plan, was not written ({unset.numel()} such in [{a}, {b}))")
        checked += b - a
    assert checked > size // 4
    eng.fill_workspace(0x00)
    clean = forward(model, x)
    for got in (first, dirty, clean):
        assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    assert torch.equal(dirty[0], clean[0]) and torch.equal(dirty[1], clean[1]), "0xFF arena and zero arena differ"
    assert torch.equal(first[0], clean[0]) and torch.equal(first[1], clean[1])
    return plan


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("dtype", DTYPES)
def test_product_forward_writes_what_its_plan_says(dtype, shape):
    plan = check_case(new_model(dtype), shape, fresh=True)
    if dtype == "fp32" and shape == SMALL:  # split-K partial sums in MID at this shape
        assert any(r["role"] == "part" for l in plan["launches"] for r in l["ranges"])


_SHARED = {}


@pytest.mark.parametrize("variant", sorted(_lib.VARIANTS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_variant_forward_writes_what_its_plan_says(dtype, variant):
    if dtype not in _SHARED:
        _SHARED[dtype] = new_model(dtype)
    m = _SHARED[dtype]
    # no_winograd needs its weight images: the only variant that has to reload
    old = m.set_kernel_variants(variant) if variant == "no_winograd" else m.engine.set_variants(variant)
    try:
        check_case(m, RAGGED, fresh=m.engine.workspace_bytes() == 0)
    finally:
        if variant == "no_winograd":
            m.set_kernel_variants(*old)
        else:
            m.engine.set_variants(*old)


def test_workspace_view_refusals():
    from clasfv_amd.model import Engine
    eng = Engine(dtype="fp32")
    lib = eng.lib
    base, size = ctypes.c_void_p(), ctypes.c_int64()
    stream = _lib.stream_ptr(None, eng.device)
    assert lib.clasfv_workspace_view(None, stream, ctypes.byref(base), ctypes.byref(size)) == -1
    assert b"null handle" in lib.clasfv_last_error()
    assert lib.clasfv_workspace_view(eng.h, stream, ctypes.byref(base), ctypes.byref(size)) == -1
    assert b"no workspace" in lib.clasfv_last_error()
    assert base.value is None and size.value == 0
    m = new_model("fp32")
    forward(m, clip(SMALL, m.engine.device))
    idle = torch.cuda.Stream(device=m.engine.device)
    assert lib.clasfv_workspace_view(m.engine.h, ctypes.c_void_p(idle.cuda_stream), ctypes.byref(base),
                                     ctypes.byref(size)) == -1
    assert b"no workspace" in lib.clasfv_last_error()
    assert m.engine.workspace_view()[1] == m.engine.workspace_bytes() > 0
    assert lib.clasfv_workspace_view(m.engine.h, _lib.stream_ptr(None, m.engine.device), None, None) == 0
