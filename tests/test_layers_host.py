"""CPU tests of the layer diagnostics' host side: the float64 layer references and recipes
(oracle/layer_ref.py) and the argument checks of the diagnostic C ABI that need no GPU."""
import ctypes

import torch
import torch.nn.functional as F

from oracle import layer_ref as LR, r2plus1d_ref


def _table():
    from clasfv_amd.arch import state_dict_spec
    return [(k, tuple(s)) for k, s in state_dict_spec().items()]


def test_integer_recipe_folds_to_exact_powers_of_two():
    sd, ks = LR.integer_state_dict(_table(), seed=3)
    assert len(ks) == 39  # 37 backbone BatchNorms and the decoder's two
    for bn, k in ks.items():
        scale, shift = LR.bn_fold(sd, bn)
        assert bool(((scale / torch.pow(2.0, k.double()) - 1).abs() < 1e-9).all())
        assert torch.equal(shift, sd[bn + ".bias"].double())  # mean 0: beta itself, an integer
    R = "r2plus1d_model."
    for name, bn in ((R + "layer4.1.conv1.0.0", R + "layer4.1.conv1.0.1"), (R + "layer3.0.conv1.0.3", R + "layer3.0.conv1.1"),
                     (R + "stem.0", R + "stem.1")):
        w = sd[name + ".weight"].double()
        scale, _ = LR.bn_fold(sd, bn)
        folded = (w * scale.view(-1, 1, 1, 1, 1)).float().double()  # as the engine folds: double product, float32
        assert torch.equal(folded, w * torch.pow(2.0, ks[bn].double()).view(-1, 1, 1, 1, 1))
        assert 0.25 < float((w == 0).double().mean()) < 0.45
        assert float(w.abs().max()) == (8 if tuple(w.shape[2:]) == (1, 3, 3) else 2)


def test_float_recipe_ranges():
    sd = LR.float_state_dict(_table(), seed=4)
    w = sd["r2plus1d_model.layer2.0.conv1.0.0.weight"]
    assert 0.5 <= float(w.abs().min()) and float(w.abs().max()) <= 1 and 0.4 < float((w > 0).float().mean()) < 0.6
    g, v = sd["r2plus1d_model.layer2.0.conv1.0.1.weight"], sd["r2plus1d_model.layer2.0.conv1.0.1.running_var"]
    assert 0.5 <= float(g.min()) and float(g.max()) <= 2 and 0.5 <= float(v.min()) and float(v.max()) <= 2


def test_conv_reference_is_conv_bn_residual_and_its_denominator_bounds_it():
    sd = LR.float_state_dict(_table(), seed=5)
    gen = torch.Generator().manual_seed(1)
    pre, bn = "r2plus1d_model.layer1.0.conv2.0.3", "r2plus1d_model.layer1.0.conv2.1"
    x = LR.signed_unit((2, 144, 4, 3, 5), gen, torch.float64)
    res = LR.signed_unit((2, 64, 4, 3, 5), gen, torch.float64)
    scale, shift = LR.bn_fold(sd, bn)
    y, den, wf = LR.conv_reference(x, sd[pre + ".weight"].double(), (1, 1, 1), (1, 0, 0), scale=scale, shift=shift,
                                   sd=sd, bn=bn, res=res)
    want = F.conv3d(x, wf, shift, 1, (1, 0, 0)) + res  # the folded form agrees with BN as written
    assert float((y - want).abs().max()) < 1e-12 * float(den.max())
    assert bool((y.abs() <= den * (1 + 1e-12)).all())
    chans = torch.tensor([3, 12, 19])
    y2, den2, _ = LR.conv_reference(x, sd[pre + ".weight"].double(), (1, 1, 1), (1, 0, 0), scale=scale, shift=shift,
                                    sd=sd, bn=bn, res=res, channels=chans)
    assert torch.equal(y2, y[:, chans]) and torch.equal(den2, den[:, chans])


def test_layouts_round_trip():
    x = torch.arange(2 * 5 * 2 * 3 * 4, dtype=torch.float32).reshape(2, 5, 2, 3, 4)
    cl = LR.to_channels_last(x, 8, torch.float32)
    assert cl.shape == (2, 2, 3, 4, 8) and bool((cl[..., 5:] == 0).all())
    assert torch.equal(LR.from_channels_last(cl, 5), x)
    c8 = LR.to_c8(F.pad(cl, (0, 8)))  # 16 channels: two 8-channel blocks
    assert c8.shape == (2, 48, 8) and float(c8[0, 7, 3]) == float(cl.reshape(48, 8)[7, 3])
    assert torch.equal(LR.from_c8(c8, (2, 2, 3, 4), 16)[..., :8], cl)
    assert float(LR.bf16_ulp(torch.tensor([1.0, 3.0, 0.75], dtype=torch.float64))[1]) == 2.0 ** -6


def test_decoder_reference_is_the_commuted_form_of_the_reference_head():
    """decoder_reference over projected taps equals r2plus1d_ref.head over the raw taps (float64)."""
    sdf = LR.float_state_dict(_table(), seed=6)
    sd = {k: v.double() for k, v in sdf.items()}
    t, h, w = 8, 16, 32
    gen = torch.Generator().manual_seed(0)
    shapes = LR.tap_shapes(t, h, w)
    assert shapes == [(8, 8, 16), (4, 4, 8), (2, 2, 4), (1, 1, 2)]
    assert LR.tap_shapes(3, 24, 32) == [(3, 12, 16), (2, 6, 8), (1, 3, 4), (1, 2, 2)]
    feat = [LR.signed_unit((1, c) + s, gen, torch.float64)
            for c, s in zip((64, 64, 128, 256, 512), [shapes[0]] + shapes)]
    rs, rm = r2plus1d_ref.head(sd, feat)
    s1, _ = LR.bn_fold(sdf, "comb_batch_norm_1")
    w1 = sd["comb_1_layer.weight"] * s1.view(-1, 1, 1, 1, 1)
    cols = [0, 64, 128, 256, 512, 1024]
    proj = [F.conv3d(f, w1[:, cols[i]:cols[i + 1]]) for i, f in enumerate(feat)]
    ds, dm = LR.decoder_reference(sdf, [proj[0] + proj[1], proj[2], proj[3], proj[4]], (t, h, w))
    assert float((ds - rs).abs().max()) <= 1e-12 * float(rs.abs().max())
    assert float((dm - rm).abs().max()) <= 1e-12


def test_diagnostic_entries_reject_a_null_handle():
    from clasfv_amd import _lib
    lib = _lib.load()
    assert lib.clasfv_conv_count(None) == -1
    assert lib.clasfv_conv_info(None, 0, None, None, None, None, None, None, None, None, None) == -1
    name = ctypes.c_char_p()
    assert lib.clasfv_run_conv(None, 0, None, 1, 1, 1, 1, None, None, 1, 0, 0, None, None, 0, ctypes.byref(name),
                               None) == -1
    assert lib.clasfv_run_decoder(None, None, None, None, None, 1, 8, 16, 16, None, None, None) == -1
    assert b"null handle" in lib.clasfv_last_error()


def test_launch_log_entries_reject_a_null_handle():
    from clasfv_amd import _lib
    lib = _lib.load()
    assert lib.clasfv_set_launch_log(None, 1) == -1
    assert b"null handle" in lib.clasfv_last_error()
    labels, grids = (ctypes.c_char_p * 4)(), (ctypes.c_int64 * 4)()
    passes, convs = (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
    assert lib.clasfv_launch_log(None, 4, labels, grids, passes, convs) == -1
    assert b"null handle" in lib.clasfv_last_error()
    assert lib.clasfv_launch_log(None, 0, None, None, None, None) == -1


def test_fill_workspace_rejects_a_null_handle():
    from clasfv_amd import _lib
    lib = _lib.load()
    assert lib.clasfv_param_info(None, 0, None, None, None) == -1  # leaves another message behind
    assert lib.clasfv_fill_workspace(None, 0xFF, None) == -1
    assert b"null handle" in lib.clasfv_last_error()
    assert lib.clasfv_workspace_bytes(None) == 0
