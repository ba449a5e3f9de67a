"""conv_dma_x3's wide form (256 output voxels x 240 output channels per block; csrc/conv.hip) against the
form it replaces on the fp32 engines' 240- and 480-channel strided convs (128 voxels x 80 / 96 channels),
which the variant bit CLASFV_VARIANT_NO_DMA_X3_WIDE restores. Everything goes through clasfv_run_conv and
clasfv_forward, so the path under test is the one the forward dispatches.

The two forms run the same products in the same order, so their outputs must be the same bits. Shapes: the
smallest at which the wide form can go wrong --
 * 64 -> 240, 1x3x3, stride (1,2,2), 1 x 2 x 10 x 10: M = 50, one partial 256-row tile, every edge tap
   invalid somewhere;
 * the same conv at 3 x 3 x 18 x 18: M = 729, two full tiles and a partial one, rows of one tile spanning
   frames and clips;
 * 128 -> 480 at 2 x 2 x 14 x 14: M = 196, two N blocks per M tile (the second block's channel offset).
conv_dma_x3 writes channels-last only (the forward never asks it for the 8-channel-blocked layout, and
clasfv_run_conv refuses it), so that is the layout tested.
"""
import pytest
import torch
import torch.nn.functional as F

from clasfv_amd import _lib
from tests import test_layers_gpu as TL

pytestmark = pytest.mark.gpu

NARROW = _lib.NO_DMA_X3_WIDE
L2, L3 = "layer2.0.conv1.0.0", "layer3.0.conv1.0.0"
SHAPES = [(L2, (1, 2, 10, 10)), (L2, (3, 3, 18, 18)), (L3, (2, 2, 14, 14))]
WIDE_TAG = "N240"  # the wide instantiations' first template argument in the launch log's labels


def shape_id(s):
    return f"{s[0]}-{'x'.join(map(str, s[1]))}"


def case(layer, nthw):
    return TL.C(layer, "fp32", nthw, "conv_dma_x3")


_BUILT = {}


def built(layer, nthw):
    """TL.build_case of the shape (inputs between guard bands and the float64 reference), computed once."""
    if (layer, nthw) not in _BUILT:
        _BUILT[(layer, nthw)] = TL.build_case(TL.net("fp32", "float"), case(layer, nthw))
    return _BUILT[(layer, nthw)]


def run(layer, nthw, relu, flags):
    """One clasfv_run_conv with the variant bits `flags`, the output between guard bands of all-ones bits.
    Returns (output bits [M, cout_p] as int32, the launch log). Asserts that the launch stayed inside the
    M x cout_p elements it was given, wrote all of them, and left its inputs alone."""
    nt = TL.net("fp32", "float")
    eng, b = nt.engine, built(layer, nthw)
    e = b["e"]
    n, to_, ho, wo = b["out"]
    m = n * to_ * ho * wo
    _, ybits, y = TL.guarded(m * e["cout_p"], torch.float32, eng.device)
    old = eng.lib.clasfv_get_kernel_variants(eng.h)
    _lib.check(eng.lib.clasfv_set_kernel_variants(eng.h, flags), "clasfv_set_kernel_variants")
    eng.set_launch_log(True)
    try:
        name = TL.on_device(lambda: (eng.run_conv(e["index"], b["x"], nthw, y, relu=relu), torch.cuda.synchronize())[0])
        log = eng.launch_log()
    finally:
        eng.set_launch_log(False)
        _lib.check(eng.lib.clasfv_set_kernel_variants(eng.h, old), "clasfv_set_kernel_variants")
    assert name == "conv_dma_x3"
    assert TL.inputs_intact(b["inputs"]), "an input or its guard bands were written"
    assert TL.guards_intact(ybits), "write outside the M x Cout output elements"
    payload = ybits[TL.GUARD:TL.GUARD + m * e["cout_p"]]
    assert bool((payload != -1).all()), "output elements left unwritten"
    return payload.clone().view(m, e["cout_p"]), log


@pytest.mark.parametrize("relu", (False, True), ids=("linear", "relu"))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_wide_form_is_bit_identical_to_the_narrow_form(shape, relu):
    """The raw output bits of the two forms are equal, each form is the one the launch log names, the wide
    form's grid is ceil(M / 256) x (Cout / 240) blocks, and (the canaries of run()) neither writes outside the
    M x Cout elements although M % 256 != 0 in every shape."""
    layer, nthw = shape
    wide, log_w = run(layer, nthw, relu, 0)
    narrow, log_n = run(layer, nthw, relu, NARROW)
    m, cout_p = wide.shape
    assert m % 256 != 0
    assert [WIDE_TAG in label for label, _, _, _ in log_w] == [True], log_w
    assert [WIDE_TAG in label for label, _, _, _ in log_n] == [False], log_n
    assert log_w[0][1] == -(-m // 256) * (cout_p // 240), log_w
    assert log_n[0][1] == -(-m // 128) * (cout_p // (80 if cout_p == 240 else 96)), log_n
    assert torch.equal(wide, narrow), f"{int((wide != narrow).sum())} of {wide.numel()} outputs differ"


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=shape_id)
def test_wide_form_against_float64(shape):
    """The wide form against the float64 direct convolution of tests/test_layers_gpu.py, under the bar its
    test_conv_float_data holds conv_dma_x3 to (the "x3" family's: error over the sum of the magnitudes of
    everything added), ReLU off and on."""
    layer, nthw = shape
    b = built(layer, nthw)
    e = b["e"]
    n, to_, ho, wo = b["out"]
    worst = 0.0
    for relu in (False, True):
        ybits, log = run(layer, nthw, relu, 0)
        assert WIDE_TAG in log[0][0]
        y = ybits.view(torch.float32).view(n, to_, ho, wo, e["cout_p"])
        got = TL.LR.from_channels_last(y, e["cout"]).double().cpu()
        ref = F.relu(b["y64"]) if relu else b["y64"]
        worst = max(worst, float(((got - ref).abs() / b["den"]).max()))
    print(f"WIDE_ERR {shape_id(shape)} e={worst:.3e} bar={TL.BARS['x3']:.3e}")
    assert worst <= TL.BARS["x3"]


def test_forward_is_bit_identical_and_runs_the_wide_form():
    """One clip of 32 x 112 x 112, seeded weights: seg and motion with and without the variant bit are the same
    bits; the forward's launch log shows layer2 block 1's strided spatial conv on the wide form with its grid
    of ceil(32 * 28 * 28 / 256) = 98 blocks (and on the narrow form's 196 x 3 with the bit set), under the
    kernel name the launch plan gives that conv with either setting (the plan records names, not grids)."""
    from clasfv_amd.model import R2plus1D_18_MotionNet, forward_plan
    model = R2plus1D_18_MotionNet(pretrained=False, dtype="fp32")
    eng = model.engine
    conv = {e["prefix"]: e["index"] for e in eng.conv_table()}[TL.R + L2]
    g = torch.Generator().manual_seed(5)
    x = torch.rand((1, 3, 32, 112, 112), generator=g).to(eng.device)
    out = {}
    for flags in (0, NARROW):
        _lib.check(eng.lib.clasfv_set_kernel_variants(eng.h, flags), "clasfv_set_kernel_variants")
        eng.set_launch_log(True)
        try:
            seg, mot = TL.on_device(lambda: model(x))
            torch.cuda.synchronize()
            log = [l for l in eng.launch_log() if l[3] == conv]
        finally:
            eng.set_launch_log(False)
            _lib.check(eng.lib.clasfv_set_kernel_variants(eng.h, 0), "clasfv_set_kernel_variants")
        out[flags] = (seg.clone(), mot.clone(), log)
        plan = [l for l in forward_plan(1, 32, 112, 112, "fp32", flags)["launches"] if l["conv"] == conv]
        assert [l["kernel"] for l in plan] == ["conv_dma_x3"]
        assert [TL.label_kernel(label) for label, _, _, _ in log] == ["conv_dma_x3"]
    m = 32 * 28 * 28
    (label_w, grid_w, _, _), (label_n, grid_n, _, _) = out[0][2][0], out[NARROW][2][0]
    assert WIDE_TAG in label_w and grid_w == -(-m // 256)
    assert WIDE_TAG not in label_n and grid_n == (m // 128) * 3
    assert bool(torch.isfinite(out[0][0]).all()) and float(out[0][0].abs().max()) > 0
    for i, what in ((0, "seg"), (1, "motion")):
        a, b = out[0][i].view(torch.int32), out[NARROW][i].view(torch.int32)
        assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} values differ"
