"""The rescaling recipe of the dynamic-range tests (oracle/layer_ref.rescale_state_dict) on the CPU: it
preserves the function bit for bit on the float32 oracle, and it reaches every conv the engine plans."""
import numpy as np
import pytest
import torch

from oracle import layer_ref as LR, r2plus1d_ref

R = "r2plus1d_model."


def conv_names():
    """State-dict prefix and BatchNorm of every conv of plan_conv_table(), in its order: the backbone as
    arch.backbone_convs() lists it, then the four column blocks of comb_1_layer (P01, P2, P3, P4)."""
    from clasfv_amd.arch import backbone_convs
    names = [(c.name, c.bn, 0, c) for _, c in backbone_convs()]
    return names + [("comb_1_layer", "comb_batch_norm_1", col0, None) for col0 in (0, 128, 256, 512)]


@pytest.fixture(scope="module")
def base():
    import clasfv_amd.weights as W
    sd = W.synthetic_state_dict(W.DEFAULT_SEED)
    x = torch.from_numpy(np.random.default_rng(3).uniform(0, 1, (1, 3, 8, 32, 32)).astype(np.float32))
    return sd, x, r2plus1d_ref.forward(sd, x)


@pytest.mark.parametrize("K", [8, 30])
def test_rescaled_weights_compute_the_same_bits_on_the_cpu_oracle(base, K):
    """Channel exponents uniform in [-K, K] on every BatchNorm, the clip and the seg head, compensated in the
    consumers' columns: the float32 oracle returns the same motion and 2^j times the same seg logits, bit for
    bit. The recipe is function-preserving, so a difference on the GPU is the engine's."""
    sd, x, (seg, mot) = base
    sd2, exps = LR.rescale_state_dict(sd, K, seed=100 + K)
    x2 = (x.double() * LR.pow2(exps["clip"]).view(1, 3, 1, 1, 1)).float()
    seg2, mot2 = r2plus1d_ref.forward(sd2, x2)
    j = LR.pow2(exps["out"]["segmentation_head"]).view(1, 2, 1, 1, 1)
    assert torch.equal(mot2, mot)
    assert torch.equal(seg2.double(), seg.double() * j)
    assert float(seg.abs().min()) > 0  # no logit hides behind a zero


def test_rescaling_leaves_no_conv_out():
    """Every conv of plan_conv_table() has a non-constant exponent vector on its input channels and on its
    output channels: a conv added to the engine later cannot be silently left out of the recipe."""
    import clasfv_amd.weights as W
    from clasfv_amd.model import plan_conv_table
    _, exps = LR.rescale_state_dict(W.synthetic_state_dict(W.DEFAULT_SEED), 30, seed=1)
    names = conv_names()
    for dtype in ("fp32", "bf16"):
        table = plan_conv_table(dtype)
        assert len(table) == len(names) == 41  # 37 backbone convs and the four projections
        for e, (conv, bn, col0, c) in zip(table, names):
            cin = e["cin"] + e["cin2"]
            if c is not None:  # the mapping by position is the engine's: same channels, kernel and stride
                assert (c.cin, c.cout, c.k, c.s, c.p) == (cin, e["cout"], e["kernel"], e["stride"], e["padding"]), conv
            kin, kout = exps["in"][conv][col0:col0 + cin], exps["out"][bn]
            assert kin.numel() == cin and kout.numel() == e["cout"], conv
            assert int(kin.min()) < int(kin.max()) and int(kout.min()) < int(kout.max()), conv
    # and nothing else: every conv weight of the state dict is a consumer, every BatchNorm a producer
    spec = W.synthetic_state_dict(W.DEFAULT_SEED)
    convs = {k[:-len(".weight")] for k, v in spec.items() if k.endswith(".weight") and np.ndim(v) == 5}
    bns = {k[:-len(".running_var")] for k in spec if k.endswith(".running_var")}
    assert set(exps["in"]) == convs
    assert set(exps["out"]) == bns | {"segmentation_head"}
    assert int(exps["clip"].min()) < int(exps["clip"].max())


def test_rescaling_is_exact_on_the_parameters():
    """Every rescaled parameter is the original times a power of two (no rounding happened), the folded
    weights and shifts of a conv move by 2^(out - in) exactly, and untouched parameters are untouched."""
    import clasfv_amd.weights as W
    sd = {k: torch.as_tensor(v) for k, v in W.synthetic_state_dict(W.DEFAULT_SEED).items()}
    sd2, exps = LR.rescale_state_dict(sd, 30, seed=2)
    for conv, bn, col0, c in conv_names()[:37]:
        s, t = LR.bn_fold(sd, bn)
        s2, t2 = LR.bn_fold(sd2, bn)
        pout = LR.pow2(exps["out"][bn])
        assert torch.equal(s2, s * pout) and torch.equal(t2, t * pout), bn
        wf = (sd[conv + ".weight"].double() * s.view(-1, 1, 1, 1, 1)).float().double()
        wf2 = (sd2[conv + ".weight"].double() * s2.view(-1, 1, 1, 1, 1)).float().double()
        assert torch.equal(wf2, wf * pout.view(-1, 1, 1, 1, 1) / LR.pow2(exps["in"][conv]).view(1, -1, 1, 1, 1)), conv
    for k in sd:
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")) or k.startswith(R + "fc.") or \
                k in ("comb_1_layer.bias", "comb_2_layer.bias", "motion_head.bias"):
            assert torch.equal(sd2[k], sd[k]), k


def test_emulations_compute_the_conv():
    """winograd_emulation (spatial F(2x2), F(4x4) with partial tiles, temporal F(4) with T % 4 != 0) and
    split2_emulation agree with the float64 conv to fp32 / 2^-16 accuracy: they emulate roundings, not another op."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(9)
    x = LR.signed_unit((2, 12, 6, 10, 14), gen).double()
    res = LR.signed_unit((2, 16, 6, 10, 14), gen).double()
    shift = LR.signed_unit((16,), gen).double()
    for shape, pad, ms in (((16, 12, 1, 3, 3), (0, 1, 1), (2, 4)), ((16, 12, 3, 1, 1), (1, 0, 0), (4,))):
        w = LR.signed_unit(shape, gen).double()
        want = F.conv3d(x, w, shift, 1, pad) + res
        den = F.conv3d(x.abs(), w.abs(), shift.abs(), 1, pad) + res.abs()
        for m in ms:
            got = LR.winograd_emulation(x, w, shift, res, m)
            e = float(((got - want).abs() / den).max())
            assert got.shape == want.shape and 0 < e < 2e-6, (shape, m, e)
    w = LR.signed_unit((8, 3, 1, 7, 7), gen).double()
    x3 = LR.signed_unit((1, 3, 2, 16, 16), gen).double()
    got = LR.split2_emulation(x3, w, shift[:8], (1, 2, 2), (0, 3, 3))
    want = F.conv3d(x3, w, shift[:8], (1, 2, 2), (0, 3, 3))
    den = F.conv3d(x3.abs(), w.abs(), shift[:8].abs(), (1, 2, 2), (0, 3, 3))
    assert 0 < float(((got - want).abs() / den).max()) < 2.0 ** -16


def test_spread_recipe_and_draw():
    from clasfv_amd.arch import state_dict_spec
    table = [(k, tuple(s)) for k, s in state_dict_spec().items()]
    sd = LR.spread_state_dict(table, seed=7)
    w = sd[R + "layer2.0.conv1.0.0.weight"].double()
    e = torch.floor(torch.log2(w.abs()))
    assert int(e.min()) == -13 and int(e.max()) == 11  # [0.5, 1) * 2^[-12, 12]
    assert bool((e.amax((2, 3, 4)) - e.amin((2, 3, 4)) <= 1).all())  # one exponent per (o, c)
    for bn in (R + "layer2.0.conv1.0.1", R + "stem.1", "comb_batch_norm_1"):
        g, v = sd[bn + ".weight"], sd[bn + ".running_var"]
        assert int((g == 0).sum()) == 2 and int((v == 0).sum()) == 2 and not bool(((g == 0) & (v == 0)).any())
        assert 0.2 < float((g < 0).float().mean()) < 0.8
        s, _ = LR.bn_fold(sd, bn)
        assert bool(torch.isfinite(s).all())
    for per_element in (False, True):
        x = LR.spread_draw(torch.Generator().manual_seed(1), per_element=per_element)((2, 16, 4, 6, 6))
        assert int((x.abs().amax((0, 2, 3, 4)) == 0).sum()) == 2
        assert 0.44 < float((x == 0).double().mean()) < 0.51  # 1 - 14/16 * 0.6 = 0.475
        ex = torch.floor(torch.log2(x.abs()))
        ex[x == 0] = float("nan")
        spread = torch.nan_to_num(ex, -99).amax((2, 3, 4)) - torch.nan_to_num(ex, 99).amin((2, 3, 4))
        live = x.abs().amax((2, 3, 4)) > 0
        assert bool((spread[live] > 1).any()) == per_element
