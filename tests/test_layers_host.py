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
LIM31, LIM32 = 1 << 31, 1 << 32


def _closed_form(dtype, t, h, w):
    """The limit that binds at the network's shapes, by DESIGN.md's "Size limits" table. fp32: layer1's
    144-channel fp32 mid tensor, (t, h/2, w/2), 8-channel-blocked for conv_winot5, which offsets it in 32-bit
    bytes, stays below 2^32 bytes (the blocked layout is one clip's choice: a batch does not switch it off).
    That is below the limit the F(4x4,3x3) convs set on their 64-channel input, 2^31 bytes (the kernels'
    "read zeros" slot), which bound the forward while a batch could. bf16: layer1's 160-channel bf16 mid
    tensor, (t, h/2, w/2), has fewer than the 2^31 elements conv_twalk_bf16 addresses. (This export used to
    answer with the decoder's limit, 2^31 floats in the P01 tap, 2.5 times as many clips: its device-less
    engine marked no bias present, so its bf16 convs were planned on other kernels than a finalized handle
    runs, whose forward has always used the limit asserted here.)"""
    vox = t * (h // 2) * (w // 2)
    assert (LIM32 - 1) // (vox * 144 * 4) <= (LIM31 - 1) // (vox * 64 * 4)
    return (LIM32 - 1) // (vox * 144 * 4) if dtype == 0 else (LIM31 - 1) // (vox * 160)


def _dma_w_bound(t, h, w):
    """The 64-channel bf16 input of layer2's first conv, (t, h/2, w/2), from one padding row and pixel (w/2 + 1
    pixels) before it, stays below the 2^31 bytes conv_dma_w's buffer DMAs address (conv_dma would take a
    larger batch, bit for bit the same, but a batch does not change a clip's kernel)."""
    return ((LIM31 - 1) // (64 * 2) - (w // 2 + 1)) // (t * (h // 2) * (w // 2))


def _decoder_bound(t, h, w):
    return (LIM31 - 1) // (t * (h // 2) * (w // 2) * 64)


def test_max_clips_at_the_product_shapes_and_which_limit_binds():
    from clasfv_amd import _lib
    lib = _lib.load()
    want = {(0, 64, 224, 224): 9, (0, 32, 112, 112): 74, (1, 64, 224, 224): 16, (1, 32, 112, 112): 133}
    for (dtype, t, h, w), n in want.items():
        assert _closed_form(dtype, t, h, w) == n
        assert lib.clasfv_max_clips(t, h, w, dtype, 0) == n
        assert lib.clasfv_clips_fit(n, t, h, w, dtype, 0) == 0
        assert lib.clasfv_clips_fit(n + 1, t, h, w, dtype, 0) == -2
        msg = lib.clasfv_last_error()
        assert (b"conv_winot: the 8-channel-blocked input" if dtype == 0 else b"conv_twalk_bf16: the batch is past") in msg, msg
    # channels-last mid tensors (no_c8): the F(4x4,3x3) convs' 64-channel input below 2^31 bytes binds instead
    for (t, h, w), n in {(64, 224, 224): 10, (32, 112, 112): 83}.items():
        no_c8 = _lib.VARIANTS["no_c8"]
        assert lib.clasfv_max_clips(t, h, w, 0, no_c8) == n == (LIM31 - 1) // (t * (h // 2) * (w // 2) * 64 * 4)
        assert lib.clasfv_clips_fit(n + 1, t, h, w, 0, no_c8) == -2 and b"conv_wino4r" in lib.clasfv_last_error()
    # bf16 without conv_twalk_bf16: conv_dma_w's 2^31 bytes bind; without conv_dma_w too, the decoder's P01 tap
    no_twalk, no_dma_w = _lib.VARIANTS["no_twalk"], _lib.VARIANTS["no_dma_w"]
    for (t, h, w), (n_w, n_dec) in {(64, 224, 224): (20, 41), (32, 112, 112): (167, 334)}.items():
        assert lib.clasfv_max_clips(t, h, w, 1, no_twalk) == n_w == _dma_w_bound(t, h, w)
        assert lib.clasfv_clips_fit(n_w + 1, t, h, w, 1, no_twalk) == -2 and b"conv_dma_w" in lib.clasfv_last_error()
        assert lib.clasfv_max_clips(t, h, w, 1, no_twalk | no_dma_w) == n_dec == _decoder_bound(t, h, w)
        assert lib.clasfv_clips_fit(n_dec + 1, t, h, w, 1, no_twalk | no_dma_w) == -2
        assert b"decoder_kernel" in lib.clasfv_last_error()
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
        assert 1 <= mc <= _decoder_bound(t, h, w)  # the decoder's tap bounds every configuration
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
