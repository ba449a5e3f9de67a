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


# ---- size limits: max_clips and the gates behind it (host arithmetic, no device) ---------------------------
LIM31 = 1 << 31


def _closed_form(dtype, t, h, w):
    """The limit that binds at the network's shapes, by DESIGN.md's "Size limits" table. fp32: the 64-channel
    fp32 input of layer1's F(4x4,3x3) convs, (t, h/2, w/2), ends below byte 2^31 (the kernels' "read zeros"
    slot). bf16: the decoder's P01 tap, 64 fp32 channels at (t, h/2, w/2), has fewer than 2^31 floats."""
    vox = t * (h // 2) * (w // 2)
    return (LIM31 - 1) // (vox * 64 * 4) if dtype == 0 else (LIM31 - 1) // (vox * 64)


def test_max_clips_at_the_product_shapes_and_which_limit_binds():
    from clasfv_amd import _lib
    lib = _lib.load()
    want = {(0, 64, 224, 224): 10, (0, 32, 112, 112): 83, (1, 64, 224, 224): 41, (1, 32, 112, 112): 334}
    for (dtype, t, h, w), n in want.items():
        assert _closed_form(dtype, t, h, w) == n
        assert lib.clasfv_max_clips(t, h, w, dtype, 0) == n
        assert lib.clasfv_clips_fit(n, t, h, w, dtype, 0) == 0
        assert lib.clasfv_clips_fit(n + 1, t, h, w, dtype, 0) == -2
        msg = lib.clasfv_last_error()
        assert (b"conv_wino4r" if dtype == 0 else b"decoder_kernel") in msg, msg
    # other clips whose layer1 maps F(4x4,3x3) serves: the same closed forms
    for t, h, w in ((8, 32, 48), (16, 80, 112), (24, 64, 64)):
        for dtype in (0, 1):
            assert lib.clasfv_max_clips(t, h, w, dtype, 0) == _closed_form(dtype, t, h, w), (dtype, t, h, w)
    # 8 x 8 maps in layer1 (<= 64 pixels) run the split-bf16 direct GEMM instead: the temporal Winograd's 2^31
    # elements of the 144-channel mid tensor bind
    assert lib.clasfv_max_clips(8, 16, 16, 0, 0) == (LIM31 - 1) // (8 * 8 * 8 * 144) == 29127


def test_clips_fit_is_monotone_in_the_batch():
    """Every limit bounds a size that grows with N: N fits exactly when N <= max_clips, whatever the variants
    (each moves the binding limit to another kernel)."""
    from clasfv_amd import _lib
    lib = _lib.load()
    V = _lib.VARIANTS
    for dtype, variants in ((0, 0), (1, 0), (0, V["no_wino4"]), (0, V["no_winograd"]), (0, V["no_dma_x3"] | V["no_wino4r"]),
                            (1, V["no_patch_bf16"]), (1, V["no_twalk"] | V["no_dma_w"])):
        t, h, w = 32, 112, 112
        mc = lib.clasfv_max_clips(t, h, w, dtype, variants)
        assert 1 <= mc <= _closed_form(1, t, h, w)  # the decoder's tap bounds every configuration
        fits = [lib.clasfv_clips_fit(n, t, h, w, dtype, variants) == 0
                for n in (1, 2, mc // 2, mc - 1, mc, mc + 1, mc + 2, 2 * mc, 10 * mc, LIM31 // (t * h * w) + 5)]
        assert fits == [True] * 5 + [False] * 5, (dtype, variants, mc, fits)


def test_max_clips_arguments_and_a_clip_no_pass_serves():
    from clasfv_amd import _lib
    lib = _lib.load()
    assert lib.clasfv_max_clips(8, 16384, 16384, 0, 0) == 0  # one clip of 2^31 voxels: M is an int
    assert lib.clasfv_max_clips(8, 16384, 16384, 1, 0) == 0
    assert lib.clasfv_max_clips(8, 8192, 16384, 0, 0) == 0   # 2^30 voxels: the stem's 48-channel tensor alone passes 2^31 elements
    assert lib.clasfv_max_clips(12, 32, 32, 0, 0) == -2 and lib.clasfv_max_clips(8, 32, 40, 0, 0) == -2
    assert lib.clasfv_max_clips(8, 32, 32, 2, 0) == -1 and lib.clasfv_max_clips(8, 32, 32, 0, 1 << 17) == -1
    assert lib.clasfv_clips_fit(0, 8, 32, 32, 0, 0) == -1
