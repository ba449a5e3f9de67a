"""ORACLE (test infrastructure only -- never imported by the product path).

Float64 CPU references for single layers of the engine (layer-level GPU tests): one conv + BatchNorm
(eval) + residual + ReLU as the reference model writes it, the decoder head over given taps, the
state-dict recipes such tests load, and the engine's tensor layouts built with torch.

Nothing here knows how the engine folds, pads, splits or transforms anything: the conv is
``F.conv3d`` in float64 on the raw weights, BatchNorm is applied as written.
"""
import torch
import torch.nn.functional as F

EPS = 1e-5


# ---- state-dict recipes -------------------------------------------------------------------------------
def _is_spatial(shape):
    return len(shape) == 5 and shape[2] == 1 and shape[3] == 3 and shape[4] == 3


def exact_bn_pool(gen, n=4096):
    """(var, gamma_k) float32 pairs, k = -1, 0, 1, whose BatchNorm scale gamma / sqrt(var + eps),
    evaluated in double from the float32 values a state dict stores, is 2^k to within 1e-9: a folded
    weight float32(w * scale) is then exactly w * 2^k for every small integer w. The scale itself is
    not exactly 2^k: a float64 reference that applies BatchNorm as written is within 1e-9 relative of
    the exact (half-integer) result, so an equality check snaps the reference to the nearest multiple of
    1/2 (after asserting that it is that close) before rounding it to the output's format."""
    var = (0.5 + 1.5 * torch.rand(n, generator=gen, dtype=torch.float64)).float()
    d = torch.sqrt(var.double() + EPS)
    keep = torch.ones(n, dtype=torch.bool)
    gam = []
    for k in (-1, 0, 1):
        g = (d * 2.0 ** k).float()
        keep &= ((g.double() / d) / 2.0 ** k - 1.0).abs() < 1e-9
        gam.append(g)
    idx = keep.nonzero().flatten()
    assert idx.numel() >= 16, "no exactly-foldable BatchNorm scales found"
    return var[idx], torch.stack(gam, 1)[idx]


def integer_state_dict(param_table, seed=0):
    """Every conv an integer problem: weights in [-2, 2] with about a third zero (1x3x3 convs: the
    same times 4, so that F(2x2,3x3)'s G g G^T is integral), BatchNorm with mean 0, integer beta in
    [-2, 2] and a scale of exactly 2^k, k in {-1, 0, 1} per channel. Returns (state dict, {bn prefix: k})."""
    gen = torch.Generator().manual_seed(seed)
    pool_var, pool_gam = exact_bn_pool(gen)
    sd, ks = {}, {}
    for name, shape in param_table:
        if name.endswith("num_batches_tracked"):
            sd[name] = torch.zeros((), dtype=torch.float32)
        elif name.endswith("running_mean"):
            sd[name] = torch.zeros(shape)
        elif name.endswith("running_var"):
            c = shape[0]
            pick = torch.randint(0, pool_var.numel(), (c,), generator=gen)
            k = torch.randint(0, 3, (c,), generator=gen)
            pre = name[: -len(".running_var")]
            sd[name] = pool_var[pick].clone()
            sd[pre + ".weight"] = pool_gam[pick, k].clone()
            ks[pre] = k - 1
        elif len(shape) == 1 and name.endswith(".bias"):
            sd[name] = torch.randint(-2, 3, shape, generator=gen).float()
        elif len(shape) >= 2:
            w = torch.randint(-2, 3, shape, generator=gen).float()
            w = w * (torch.rand(shape, generator=gen) > 0.2)  # 1/5 of [-2,2] is 0 already: ~ a third zero
            sd[name] = w * 4 if _is_spatial(shape) else w
    for name, shape in param_table:  # BN gammas were written with their running_var
        assert name in sd, name
    return sd, ks


def signed_unit(shape, gen, dtype=torch.float32):
    """Random signs, magnitudes uniform in [0.5, 1]."""
    mag = 0.5 + 0.5 * torch.rand(shape, generator=gen, dtype=torch.float64)
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    return (mag * sign).to(dtype)


def float_state_dict(param_table, seed=0):
    """Signed weights with magnitudes in [0.5, 1]; BatchNorm gamma, var in [0.5, 2], mean, beta in [-1, 1]."""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in param_table:
        if name.endswith("num_batches_tracked"):
            sd[name] = torch.zeros((), dtype=torch.float32)
        elif name.endswith("running_var") or (len(shape) == 1 and name.endswith(".weight")):
            sd[name] = (0.5 + 1.5 * torch.rand(shape, generator=gen)).float()
        elif name.endswith("running_mean") or (len(shape) == 1 and name.endswith(".bias")):
            sd[name] = (2 * torch.rand(shape, generator=gen) - 1).float()
        else:
            sd[name] = signed_unit(shape, gen)
    return sd


# ---- one conv -----------------------------------------------------------------------------------------
def bn_fold(sd, bn):
    """(scale, shift) of an eval BatchNorm in double from the stored float32 values."""
    s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + EPS)
    return s, sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s


def bn_eval(sd, bn, x):
    """BatchNorm3d (eval) as written, in the dtype of x (float64)."""
    v = lambda k: sd[bn + k].to(x.dtype).view(1, -1, 1, 1, 1)
    return (x - v(".running_mean")) / torch.sqrt(v(".running_var") + EPS) * v(".weight") + v(".bias")


def to_bf16(x):
    """Round to nearest even bf16, returned in float64."""
    return x.float().bfloat16().double()


def bf16_ulp(y):
    """One bf16 unit in the last place of |y| (float64 tensor)."""
    e = torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def conv_reference(x, w, stride, padding, scale=None, shift=None, sd=None, bn=None, res=None, channels=None):
    """Pre-activation float64 reference and the error measure's denominator for one conv.

    x (N,Cin,T,H,W), w (Cout,Cin,kt,kh,kw), res (N,Cout,To,Ho,Wo) or None, all float64. With sd / bn the
    BatchNorm is applied as written after a raw-weight conv3d; otherwise (bf16 engines, projections)
    w is the folded weight the kernel sees and `shift` the folded bias. `scale`, `shift` (double, per
    output channel; shift may be None) are the folding, used for the denominator
    conv3d(|x|, |w * scale|) + |shift| + |res|. `channels`: compute these output channels only."""
    if channels is not None:
        w = w[channels]
        scale = scale[channels] if scale is not None else None
        shift = shift[channels] if shift is not None else None
        res = res[:, channels] if res is not None else None
    y = F.conv3d(x, w, None, stride, padding)
    if bn is not None:
        sub = {k: (v[channels] if channels is not None and v.dim() == 1 else v) for k, v in sd.items()
               if k.startswith(bn + ".")}
        y = bn_eval(sub, bn, y)
        wf = w * scale.view(-1, 1, 1, 1, 1)
    else:
        wf = w
        if shift is not None:
            y = y + shift.view(1, -1, 1, 1, 1)
    den = F.conv3d(x.abs(), wf.abs(), None, stride, padding)
    if shift is not None:
        den = den + shift.abs().view(1, -1, 1, 1, 1)
    if res is not None:
        y = y + res
        den = den + res.abs()
    return y, den, wf


# ---- the engine's tensor layouts ----------------------------------------------------------------------
def to_channels_last(x, cp, dtype):
    """(N,C,T,H,W) -> (N,T,H,W,cp) zero padded."""
    x = x.permute(0, 2, 3, 4, 1)
    return F.pad(x, (0, cp - x.shape[-1])).to(dtype).contiguous()


def to_c8(x_cl):
    """(N,T,H,W,cp) -> 8-channel-blocked [cp/8][N*T*H*W][8]."""
    cp = x_cl.shape[-1]
    return x_cl.reshape(-1, cp // 8, 8).permute(1, 0, 2).contiguous()


def from_c8(y, nthw, cp):
    n, t, h, w = nthw
    return y.reshape(cp // 8, n * t * h * w, 8).permute(1, 0, 2).reshape(n, t, h, w, cp)


def from_channels_last(y_cl, c):
    """(N,T,H,W,cp) -> (N,c,T,H,W)."""
    return y_cl[..., :c].permute(0, 4, 1, 2, 3)


def out_dim(d, k, s, p):
    return (d + 2 * p - k) // s + 1


# ---- the decoder head ---------------------------------------------------------------------------------
def tap_shapes(t, h, w):
    """Resolutions of the four projected taps (stem+layer1, layer2, layer3, layer4) for a (T,H,W) clip:
    the stem halves H and W, every later layer halves T, H and W (k 3, stride 2, pad 1)."""
    half = lambda d: (d - 1) // 2 + 1
    out = [(t, half(h), half(w))]
    for _ in range(3):
        a, b, c = out[-1]
        out.append((half(a), half(b), half(c)))
    return out


def decoder_reference(sd, taps, size):
    """The head of the reference model in float64 over already-projected taps (N,64,t,h,w): comb_1 in
    its commuted form is sum_i upsample(P_i) + BN1 shift of the comb_1 bias, where P_i already carries
    W_i and BN1's scale; then ReLU, comb_2, BN, ReLU, the two heads, tanh on motion."""
    s1, t1 = bn_fold(sd, "comb_batch_norm_1")
    h = sum(F.interpolate(p, size=size, mode="trilinear", align_corners=True) for p in taps)
    h = F.relu(h + (s1 * sd["comb_1_layer.bias"].double() + t1).view(1, -1, 1, 1, 1))
    h = F.conv3d(h, sd["comb_2_layer.weight"].double(), sd["comb_2_layer.bias"].double())
    h = F.relu(bn_eval(sd, "comb_batch_norm_2", h))
    seg = F.conv3d(h, sd["segmentation_head.weight"].double(), sd["segmentation_head.bias"].double())
    mot = torch.tanh(F.conv3d(h, sd["motion_head.weight"].double(), sd["motion_head.bias"].double()))
    return seg, mot
