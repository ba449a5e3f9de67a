"""No result depends on memory the call was not given, and the handle's state machine does what the header says.

The engine carves every activation, mid tensor, split-K partial sum, decoder tap and the decoder's index
table out of one arena per launch stream (csrc/engine.hip: make_layout, acquire_ctx), reuses it across
shapes as it stands, and gets it from hipMalloc, whose bytes are unspecified. clasfv_fill_workspace lets
a test choose those bytes: 0xFF in every byte is a NaN in fp32 and in bf16, so a kernel that reads a
line, a halo, a padded K column or a partial sum nobody wrote gives NaN or another bit pattern than the
same forward over an arena of zeros. Finiteness alone would not do: a ReLU written as a maximum turns a
NaN into 0 (pack_input_kernel without its zero lane gives finite, different outputs), so every check is
a bit comparison between fills.

 a. forward, fill 0xFF, forward, fill 0x00, forward: bit-equal and finite, for the product kernels at four
    shapes and for every A/B variant at one, both dtypes; the launch log proves which kernels ran dirty;
 b. the same clip gives the same bits whatever shapes the handle served before it;
 c. the decoder alone, whose index table lives in the arena;
 d. variant bits take effect without a finalize (NO_WINOGRAD: refuses until one);
 e. every refusal of the lifecycle comes back as its code, with its message, before anything is launched;
 f. a second finalize with other weights, another dtype or other weight images leaves nothing of the first.
"""
import ctypes

import numpy as np
import pytest
import torch

from clasfv_amd import _lib
from oracle import layer_ref as LR
from tests import test_layers_gpu as TL

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "bf16")
EINVAL, EBADSHAPE, ENOTREADY = -1, -2, -3
SMALL = (1, 3, 8, 16, 32)      # layer4 is a 1x1x2 map: split-K
RAGGED = (2, 3, 16, 64, 48)    # 48 / 16 is odd: ragged tiles
FIVE = (3, 3, 24, 80, 112)     # layer2 has five tile columns, T % 16 != 0
CLIP = (1, 3, 32, 112, 112)    # the product clip
SHAPES = (SMALL, RAGGED, FIVE, CLIP)


def shape_id(s):
    return "x".join(map(str, s))


def clip(shape, device):
    rng = np.random.default_rng(sum(shape) + 7)
    return torch.from_numpy(rng.uniform(0, 1, shape).astype(np.float32)).to(device)


def new_model(dtype, seed=None):
    from clasfv_amd.model import R2plus1D_18_MotionNet
    from clasfv_amd.weights import DEFAULT_SEED
    return R2plus1D_18_MotionNet(pretrained=False, dtype=dtype, seed=DEFAULT_SEED if seed is None else seed)


_MODELS = {}


@pytest.fixture(scope="module", params=DTYPES)
def net(request):
    """(dtype, model): one model per dtype for the whole module, product variants."""
    return request.param, shared_model(request.param)


def shared_model(dtype):
    if dtype not in _MODELS:
        _MODELS[dtype] = new_model(dtype)
    return _MODELS[dtype]


def forward(model, x):
    """(seg, motion) of one synchronised forward; a HIP error ends the session (TL.on_device)."""
    def run():
        out = model(x)
        torch.cuda.synchronize()
        return out
    return TL.on_device(run)


def fill(model, byte):
    model.engine.fill_workspace(byte)


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def finite(a):
    return bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())


_REFERENCE = {}


def reference(dtype, shape):
    """The product forward of `shape` on the module's model of `dtype`, computed once (whatever its arena
    held then) and left unchanged: what every other handle and history must reproduce bit for bit."""
    if (dtype, shape) not in _REFERENCE:
        m = shared_model(dtype)
        assert m.engine.set_variants() == ()
        _REFERENCE[(dtype, shape)] = forward(m, clip(shape, m.engine.device))
    return _REFERENCE[(dtype, shape)]


# ---- a. the arena's contents ----------------------------------------------------------------------------
_DIRTY = {}  # (dtype, shape, variant) -> (kernel names launched before any fill, after a fill)


def kernels_of(log):
    return {TL.label_kernel(label) for label, _, _, _ in log}


def dirty_arena_case(dtype, shape, variant):
    """Forward, fill 0xFF, forward, fill 0x00, forward with the asserts of (a); records what ran."""
    if (dtype, shape, variant) in _DIRTY:
        return
    m = shared_model(dtype)
    eng = m.engine
    x = clip(shape, eng.device)
    if variant == "no_winograd":  # needs its weight images: the only variant that has to reload
        old = m.set_kernel_variants(variant)
    else:
        old = eng.set_variants(*([variant] if variant else []))
    eng.set_launch_log(True)
    try:
        r0 = forward(m, x)
        before = kernels_of(eng.launch_log())
        fill(m, 0xFF)
        r1 = forward(m, x)
        after = kernels_of(eng.launch_log())
        fill(m, 0x00)
        r2 = forward(m, x)
        after |= kernels_of(eng.launch_log())
    finally:
        eng.set_launch_log(False)
        if variant == "no_winograd":
            m.set_kernel_variants(*old)
        else:
            eng.set_variants(*old)
    assert finite(r0) and finite(r1) and finite(r2), "a non-finite output"
    assert same(r0, r1), "the forward over an arena of 0xFF bytes differs from the one before it"
    assert same(r1, r2), "the forward over an arena of zeros differs from the one over 0xFF bytes"
    if not variant:
        assert same(r0, reference(dtype, shape))
    _DIRTY[(dtype, shape, variant)] = (before, after)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_forward_is_independent_of_the_arena_contents(net, shape):
    dirty_arena_case(net[0], shape, "")


@pytest.mark.parametrize("variant_name", sorted(_lib.VARIANTS))
def test_variant_forward_is_independent_of_the_arena_contents(net, variant_name):
    dirty_arena_case(net[0], RAGGED, variant_name)


def test_every_product_kernel_ran_over_a_dirty_arena():
    """Over the product cases of (a), split_sum_kernel (the split-K partial sums in "the rest of MID") and
    every kernel a product forward launches, in either dtype, were launched after a fill."""
    before, after = set(), set()
    for dtype in DTYPES:
        for shape in SHAPES:
            dirty_arena_case(dtype, shape, "")
            b, a = _DIRTY[(dtype, shape, "")]
            before |= b
            after |= a
        # the log is wired to the forward: kernels every forward of the dtype must launch
        must = {"pack_input_kernel", "conv_wino4r", "conv_stem_x3"} if dtype == "fp32" else {"pack_input_kernel",
                                                                                              "conv_stem_bf16"}
        assert must <= before, f"{dtype}: the launch log misses {sorted(must - before)}"
    print("DIRTY_ARENA kernels launched after a fill:", sorted(after))
    assert "?" not in after
    assert "split_sum_kernel" in after, "no split-K launch read the scratch after a fill"
    assert before <= after, f"never launched after a fill: {sorted(before - after)}"


# ---- b. the shape history ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_is_independent_of_the_shape_history(dtype):
    """A, B, A, C, A on a fresh handle and one stream, the arena filled with 0xFF before each forward (before
    the very first the stream has no arena: that forward runs over what hipMalloc returned, and is repeated
    over the fill)."""
    m = new_model(dtype)
    dev = m.engine.device
    assert m.engine.workspace_bytes() == 0
    first = forward(m, clip(RAGGED, dev))
    assert finite(first)
    seen, sizes = {}, [m.engine.workspace_bytes()]
    assert sizes[0] > 0
    for shape in (RAGGED, CLIP, RAGGED, SMALL, RAGGED):
        fill(m, 0xFF)
        r = forward(m, clip(shape, dev))
        assert finite(r), shape
        sizes.append(m.engine.workspace_bytes())
        if shape in seen:  # a repeat: the same bits, the same arena
            assert same(r, seen[shape]), f"{shape_id(shape)} changed with the shapes served before it"
            assert sizes[-1] == sizes[-2]
        seen.setdefault(shape, r)
        assert same(r, reference(dtype, shape)), f"{shape_id(shape)} differs from the module's handle"
    assert same(first, seen[RAGGED])
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[1] == sizes[0], "a repeat of the first shape changed the arena"
    assert sizes[2] > sizes[1], "the product clip did not grow the arena"
    assert sizes[4] == sizes[2], "a smaller shape changed the arena"


# ---- c. the decoder alone -----------------------------------------------------------------------------------
def test_decoder_alone_is_independent_of_the_arena_contents(net):
    dtype, m = net
    eng, dev = m.engine, m.engine.device
    n, t, h, w = nthw = (2, 4, 16, 32)
    gen = torch.Generator().manual_seed(t * 1000 + h * 10 + w)
    taps = [LR.to_channels_last(LR.signed_unit((n, 64) + s, gen, torch.float32), 64, torch.float32).to(dev)
            for s in LR.tap_shapes(t, h, w)]

    def run():
        seg = torch.full((n * 2 * t * h * w,), float("nan"), device=dev)
        mot = torch.full((n * 4 * t * h * w,), float("nan"), device=dev)
        TL.on_device(lambda: (eng.run_decoder(taps, nthw, seg, mot), torch.cuda.synchronize()))
        return seg, mot

    r0 = run()
    fill(m, 0xFF)
    r1 = run()
    assert finite(r0) and finite(r1)
    assert same(r0, r1), "the decoder over an arena of 0xFF bytes differs"
    fill(m, 0xFF)
    assert same(forward(m, clip(SMALL, dev)), reference(dtype, SMALL))  # another shape's index table and layout
    r2 = run()
    assert finite(r2) and same(r0, r2), "the decoder after a forward of another shape differs"


# ---- d. variant bits without a finalize -----------------------------------------------------------------------
@pytest.mark.parametrize("variant_name", sorted(_lib.VARIANTS))
def test_variant_bit_applies_without_a_finalize(net, variant_name):
    dtype, m = net
    eng = m.engine
    x = clip(RAGGED, eng.device)
    if variant_name == "no_winograd":
        old = eng.set_variants(variant_name)
        eng.set_launch_log(True)
        try:
            with pytest.raises(RuntimeError, match=r"clasfv_forward failed \(-3\)"):
                m(x)
            assert eng.launch_log() == []
            m.set_kernel_variants(variant_name)  # reloads: the direct-conv weight images exist now
            r = forward(m, x)
            assert finite(r)
            assert "conv_wino4r" not in kernels_of(eng.launch_log())
        finally:
            eng.set_launch_log(False)
            m.set_kernel_variants(*old)
        assert same(forward(m, x), reference(dtype, RAGGED))
        return
    old = eng.set_variants(variant_name)
    try:
        applied = forward(m, x)
        m.set_kernel_variants(variant_name)  # the same bits, with a reload
        reloaded = forward(m, x)
    finally:
        eng.set_variants(*old)
    assert finite(applied)
    assert same(applied, reloaded), f"{variant_name}: set without a reload differs from set with one"


# ---- e. lifecycle and refusals ----------------------------------------------------------------------------------
class Raw:
    """A fresh handle driven through ctypes, with the launch log on: refused() asserts code, message, no launch."""

    def __init__(self, dtype):
        from clasfv_amd.model import Engine
        self.L = _lib
        self.eng = Engine(dtype=dtype)
        self.lib, self.h, self.dev = self.eng.lib, self.eng.h, self.eng.device
        self.eng.set_launch_log(True)
        self.stream = _lib.stream_ptr(None, self.dev)

    def refused(self, rc, code, message):
        assert rc == code, f"returned {rc}, expected {code}: {self.lib.clasfv_last_error()}"
        err = self.lib.clasfv_last_error().decode()
        assert err and message in err, f"message {err!r} does not mention {message!r}"
        assert self.eng.launch_log() == [], "a refused call launched a kernel"

    def load(self, name, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        return self.lib.clasfv_load_param(self.h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size)

    def forward_rc(self, x, seg, mot, n=None):
        p = lambda a: self.L.ptr(a) if a is not None else None
        return self.lib.clasfv_forward(self.h, p(x), RAGGED[0] if n is None else n, *RAGGED[2:], p(seg), p(mot),
                                       self.stream)

    def outputs(self):
        n, _, t, h, w = RAGGED
        return (torch.full((n, 2, t, h, w), float("nan"), device=self.dev),
                torch.full((n, 4, t, h, w), float("nan"), device=self.dev))

    def forward(self):
        """(seg, mot) of the RAGGED clip, or the code clasfv_forward refused it with (outputs then untouched)."""
        x = clip(RAGGED, self.dev)
        seg, mot = self.outputs()
        rc = TL.on_device(lambda: (self.forward_rc(x, seg, mot), torch.cuda.synchronize())[0])
        if rc:
            assert bool(torch.isnan(seg).all()) and bool(torch.isnan(mot).all()), "a refused forward wrote its outputs"
            return rc
        self.eng.launch_log()
        return seg, mot


def test_nothing_runs_before_load_and_finalize(synthetic_sd):
    r = Raw("fp32")
    dev = r.dev
    x = clip(RAGGED, dev)
    seg, mot = r.outputs()
    taps = [torch.zeros((1,) + s + (64,), device=dev) for s in LR.tap_shapes(8, 16, 16)]
    name = ctypes.c_char_p()
    names = [n for n, _ in r.eng.param_table()]
    # before any load
    r.refused(r.forward_rc(x, seg, mot), ENOTREADY, "finalize")
    r.refused(r.lib.clasfv_run_conv(r.h, 0, r.L.ptr(x), 1, 8, 16, 16, None, None, 1, 0, 0, r.L.ptr(seg), None, 0,
                                    ctypes.byref(name), r.stream), ENOTREADY, "finalize")
    r.refused(r.lib.clasfv_run_decoder(r.h, *[r.L.ptr(a) for a in taps], 1, 8, 16, 16, r.L.ptr(seg), r.L.ptr(mot),
                                       r.stream), ENOTREADY, "finalize")
    r.refused(r.lib.clasfv_finalize(r.h), ENOTREADY, "parameter not loaded: " + names[0])
    # everything but the classifier, num_batches_tracked with no element or one: still one parameter short
    last = "segmentation_head.bias"
    tracked = 0
    for k, v in synthetic_sd.items():
        if ".fc." in k or k == last:
            continue
        if k.endswith("num_batches_tracked"):
            tracked += 1
            rc = r.lib.clasfv_load_param(r.h, k.encode(), None, 0) if tracked % 2 else r.load(k, np.zeros(1))
        else:
            rc = r.load(k, v)
        assert rc == 0, (k, r.lib.clasfv_last_error())
    assert tracked == 39
    r.refused(r.lib.clasfv_finalize(r.h), ENOTREADY, "parameter not loaded: " + last)
    assert r.load(last, synthetic_sd[last]) == 0
    # fully loaded, not finalized
    r.refused(r.forward_rc(x, seg, mot), ENOTREADY, "finalize")
    torch.cuda.synchronize()
    assert bool(torch.isnan(seg).all()) and bool(torch.isnan(mot).all())
    assert r.eng.workspace_bytes() == 0
    assert r.lib.clasfv_finalize(r.h) == 0, r.lib.clasfv_last_error()
    assert same(r.forward(), reference("fp32", RAGGED)), "a handle loaded without the classifier differs"


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_a_ready_handle_as_it_was(dtype, synthetic_sd):
    other = "bf16" if dtype == "fp32" else "fp32"
    r = Raw(dtype)
    r.eng.load(synthetic_sd)
    r0 = r.forward()
    assert same(r0, reference(dtype, RAGGED))
    x = clip(RAGGED, r.dev)
    seg, mot = r.outputs()
    w_name = "r2plus1d_model.layer2.0.conv1.0.0.weight"
    w = np.asarray(synthetic_sd[w_name], dtype=np.float32)

    def still_ready():
        assert same(r.forward(), r0)

    # refused loads keep the handle ready
    r.refused(r.load("r2plus1d_model.layer9.weight", w), EINVAL, "unknown parameter")
    still_ready()
    r.refused(r.load(w_name, w.reshape(-1)[:-1]), EINVAL, "size mismatch")
    still_ready()
    r.refused(r.lib.clasfv_load_param(r.h, w_name.encode(), None, w.size), EINVAL, "null data")
    still_ready()
    # a load that succeeds needs a finalize, even of the values the handle already has
    assert r.load(w_name, w) == 0
    r.refused(r.forward_rc(x, seg, mot), ENOTREADY, "finalize")
    assert r.forward() == ENOTREADY
    r.eng.launch_log()
    assert r.lib.clasfv_finalize(r.h) == 0
    still_ready()
    # dtype: the current one keeps the handle ready, an unknown one is refused, the other needs a finalize
    assert r.lib.clasfv_set_compute_dtype(r.h, r.L.DTYPES[dtype]) == 0
    still_ready()
    r.refused(r.lib.clasfv_set_compute_dtype(r.h, 7), EINVAL, "unknown dtype")
    assert r.lib.clasfv_get_compute_dtype(r.h) == r.L.DTYPES[dtype]
    still_ready()
    assert r.lib.clasfv_set_compute_dtype(r.h, r.L.DTYPES[other]) == 0
    r.refused(r.forward_rc(x, seg, mot), ENOTREADY, "finalize")
    assert r.lib.clasfv_finalize(r.h) == 0
    assert same(r.forward(), reference(other, RAGGED))
    assert r.lib.clasfv_set_compute_dtype(r.h, r.L.DTYPES[dtype]) == 0
    r.refused(r.forward_rc(x, seg, mot), ENOTREADY, "finalize")
    assert r.lib.clasfv_finalize(r.h) == 0
    still_ready()
    # forward's own arguments (the shapes it has no tiles for: tests/test_gpu.py)
    r.refused(r.forward_rc(None, seg, mot), EINVAL, "null tensor")
    r.refused(r.forward_rc(x, None, mot), EINVAL, "null tensor")
    r.refused(r.forward_rc(x, seg, None), EINVAL, "null tensor")
    r.refused(r.forward_rc(x, seg, mot, n=0), EINVAL, "N must be")
    still_ready()
    # the workspace fill
    idle = torch.cuda.Stream(device=r.dev)
    r.refused(r.lib.clasfv_fill_workspace(r.h, 0xFF, ctypes.c_void_p(idle.cuda_stream)), EINVAL, "no workspace")
    still_ready()
    r.refused(r.lib.clasfv_fill_workspace(r.h, 256, r.stream), EINVAL, "fill byte")
    still_ready()
    r.refused(r.lib.clasfv_fill_workspace(r.h, -1, r.stream), EINVAL, "fill byte")
    still_ready()
    assert r.lib.clasfv_fill_workspace(r.h, 0xFF, r.stream) == 0
    still_ready()
    torch.cuda.synchronize()
    assert bool(torch.isnan(seg).all()) and bool(torch.isnan(mot).all()), "a refused forward wrote its outputs"


# ---- f. re-finalize round trips -----------------------------------------------------------------------------------
SEED_B = 4321


def as_tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


@pytest.mark.parametrize("dtype", DTYPES)
def test_refinalize_with_other_weights_and_back(dtype, synthetic_sd):
    import clasfv_amd.weights as W
    sd_b = W.synthetic_state_dict(SEED_B)
    m = new_model(dtype)
    x = clip(RAGGED, m.engine.device)
    a1 = forward(m, x)
    assert same(a1, reference(dtype, RAGGED))
    m.load_state_dict(as_tensors(sd_b))
    b = forward(m, x)
    m.load_state_dict(as_tensors(synthetic_sd))
    a2 = forward(m, x)
    assert finite(b)
    assert not torch.equal(b[0], a1[0]) and not torch.equal(b[1], a1[1]), "other weights, the same result"
    assert same(a2, a1), "weights A, B, A: the third result differs from the first"
    assert same(b, forward(new_model(dtype, seed=SEED_B), x)), "weights B after A differ from B on a fresh handle"


@pytest.mark.parametrize("dtype", DTYPES)
def test_refinalize_with_one_projection_tensor_changed(dtype, synthetic_sd):
    """comb_1_layer.weight alone: finalize_projections rebuilds the four tap projections' images, whose
    pointers travel through a temporary Conv."""
    name = "comb_1_layer.weight"
    gen = np.random.default_rng(5)
    w = np.asarray(synthetic_sd[name], dtype=np.float32)
    changed = dict(synthetic_sd)
    changed[name] = (w * gen.uniform(0.5, 1.5, w.shape)).astype(np.float32)
    m = new_model(dtype)
    x = clip(RAGGED, m.engine.device)
    a = forward(m, x)
    m.load_state_dict({name: torch.from_numpy(changed[name])}, strict=False)
    c = forward(m, x)
    assert finite(c)
    assert not torch.equal(c[0], a[0]) and not torch.equal(c[1], a[1]), "comb_1 changed, the result did not"
    fresh = new_model(dtype)
    fresh.load_state_dict(as_tensors(changed))
    assert same(c, forward(fresh, x)), "comb_1 changed on a used handle differs from a fresh handle"
    m.load_state_dict({name: torch.from_numpy(w)}, strict=False)
    assert same(forward(m, x), a)


def test_refinalize_in_the_other_dtype_and_back():
    m = new_model("fp32")
    x = clip(RAGGED, m.engine.device)
    a1 = forward(m, x)
    m.set_compute_dtype("bf16")
    b = forward(m, x)
    m.set_compute_dtype("fp32")
    a2 = forward(m, x)
    assert same(a1, reference("fp32", RAGGED))
    assert same(b, reference("bf16", RAGGED)), "bf16 after fp32 on one handle differs from a bf16 handle"
    assert same(a2, a1), "fp32, bf16, fp32: the third result differs from the first"


@pytest.mark.parametrize("dtype", DTYPES)
def test_refinalize_without_winograd_and_back(dtype):
    m = new_model(dtype)
    x = clip(RAGGED, m.engine.device)
    a1 = forward(m, x)
    m.set_kernel_variants("no_winograd")
    d = forward(m, x)
    m.set_kernel_variants()
    a2 = forward(m, x)
    assert finite(d)
    assert same(a1, reference(dtype, RAGGED))
    assert same(a2, a1), "no_winograd on, then off: the result differs from the first"
