"""The raw-patch ring of the F(4x4,3x3) kernels at the shapes where its staging can go wrong.

conv_wino4r stages whole 128-B pixel lines: a ring stage holds four 8-channel chunks (32 input channels) of
the tile group's patch, two stages per block, and chunk k reads its 32 B at k % 4 * 32 inside the pixel's
row. conv_wino4w and conv_wino4 stage one chunk at a time in two 4-channel regions. The three compute the
same products in the same order from the same U values, so on the same inputs their outputs must be
bit-equal: a wrong slot, part or stage offset in one of them shows as a bit difference even where it stays
under the float bar.

Per case, on one set of inputs and one float64 reference (tests/test_layers_gpu.py's builders):
 * each kernel under the wino4 family bar of test_layers_gpu (BARS["wino4"]), ReLU off and on, with that
   file's memory discipline (guard bands around the output and around x, whose whole-line staging must
   not carry a byte from outside it into a kept output; every element written, padded channels +0);
 * the three outputs bit-equal.
Integer data (two cases): every kernel's output snapped to the nearest multiple of 1/2 equals the exact
result, so a channel fetched from the wrong place is an exact mismatch.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import test_layers_gpu as TL

pytestmark = pytest.mark.gpu

KERNELS = (("conv_wino4r", ()), ("conv_wino4w", ("no_wino4r",)), ("conv_wino4", ("no_wino4w",)))
L1, L2, L3 = "layer1.0.conv1.0.0", "layer2.1.conv1.0.0", "layer3.1.conv1.0.0"  # Cin 64 / 128 / 256

# (layer, (N, T, H, W), y_c8). Stages per block: Cin 64 two (the whole patch, no refill), 128 one refill
# per ring buffer, 256 the ring wraps twice. Maps of <= 64 pixels reach these kernels only for the
# 8-channel-blocked consumer (pick_kernel), hence y_c8 there.
SHAPES = [
    # 14x14: partial edge tiles both ways, 4 x 4 tile groups
    (L1, (2, 4, 14, 14), False), (L2, (2, 4, 14, 14), False), (L3, (2, 4, 14, 14), False),
    # 7x7: partial tiles, 8 x 2 groups of four frames
    (L1, (2, 4, 7, 7), True), (L3, (2, 4, 7, 7), True),
    # 2 clips x 3 frames: 8x8 -> 6 x 2 groups (12 tiles) over three frames; 12x20 -> 3 x 5 (15 tiles)
    (L1, (2, 3, 8, 8), True), (L2, (2, 3, 8, 8), True),
    (L2, (2, 3, 12, 20), False), (L3, (2, 3, 12, 20), False),
    # one clip, the product's layer1 groups (8 rows x 2 tiles of a 14-tile row) and layer2's (16 x 1 of a
    # 7-tile row: the largest stage, 74 KiB)
    (L1, (1, 2, 16, 56), False), (L2, (1, 4, 16, 28), False),
    # three clips: 9 groups, a block count that is no multiple of the 8 XCDs
    (L1, (3, 3, 12, 20), False),
]
INT_SHAPES = [(L1, (2, 4, 14, 14), False), (L1, (1, 2, 16, 56), False)]


def _case(layer, nthw, y_c8, kernel, flags):
    return TL.C(layer, "fp32", nthw, kernel, flags, y_c8=y_c8)


def _id(s):
    layer, (n, t, h, w), y_c8 = s
    return f"{layer}-{n}x{t}x{h}x{w}" + ("-yc8" if y_c8 else "")


def _bits(full):
    return full.contiguous().view(torch.int32)


@pytest.mark.parametrize("s", SHAPES, ids=_id)
def test_ring_float_data_three_kernels(s):
    layer, nthw, y_c8 = s
    nt = TL.net("fp32", "float")
    # one set of inputs and one reference for the three kernels: the case id seeds build_case's generator
    b = TL.build_case(nt, _case(layer, nthw, y_c8, "conv_wino4r", ()))
    for relu in (False, True):
        ref = F.relu(b["y64"]) if relu else b["y64"]
        outs = {}
        for kernel, flags in KERNELS:
            y, _, full = TL.launch(nt, _case(layer, nthw, y_c8, kernel, flags), b, relu)
            e = float(((y - ref).abs() / b["den"]).max())
            print(f"RING_ERR {kernel} {_id(s)} relu={int(relu)} e={e:.3e}")
            assert e <= TL.BARS["wino4"], f"{kernel}: e = {e:.3e} above the wino4 bar {TL.BARS['wino4']:.3e}"
            outs[kernel] = _bits(full)
        for kernel in ("conv_wino4w", "conv_wino4"):
            diff = int((outs[kernel] != outs["conv_wino4r"]).sum())
            assert diff == 0, f"relu={relu}: {kernel} differs from conv_wino4r in {diff} of {outs[kernel].numel()} outputs"


@pytest.mark.parametrize("s", INT_SHAPES, ids=_id)
def test_ring_integer_data_three_kernels(s):
    """test_layers_gpu's integer recipe: inputs in [-2, 2], 1x3x3 weights multiples of 4 in [-8, 8], BatchNorm
    scales 2^k, so the exact result is a multiple of 1/2 and every product one of magnitude >= 2. F(4x4,3x3)
    is not exact on such data (its G has sixths), but its error is bounded by the family bar times the sum of
    magnitudes den; the test asserts bar * max(den) < 1/4, so a correct kernel's output snaps to the exact
    result, and one that reads a channel from the wrong slot is off by whole products."""
    layer, nthw, y_c8 = s
    nt = TL.net("fp32", "int")
    b = TL.build_case(nt, _case(layer, nthw, y_c8, "conv_wino4r", ()))
    assert TL.BARS["wino4"] * float(b["den"].max()) < 0.25
    exact = torch.round(b["y64"] * 2) / 2
    assert float((b["y64"] - exact).abs().max()) <= 2e-9 * float(b["y64"].abs().max()) + 1e-12
    outs = {}
    for kernel, flags in KERNELS:
        y, _, full = TL.launch(nt, _case(layer, nthw, y_c8, kernel, flags), b, False)
        bad = torch.round(y * 2) / 2 != exact
        print(f"RING_INT {kernel} {_id(s)} max|d|={float((y - exact).abs().max()):.3e}")
        assert not bool(bad.any()), f"{kernel}: {int(bad.sum())} of {bad.numel()} outputs snap to another value"
        outs[kernel] = _bits(full)
    for kernel in ("conv_wino4w", "conv_wino4"):
        assert torch.equal(outs[kernel], outs["conv_wino4r"]), f"{kernel} differs from conv_wino4r"
