"""ORACLE (test infrastructure only -- never imported by the product path).

Float64 CPU references for single layers of the engine (layer-level GPU tests): one conv + BatchNorm
(eval) + residual + ReLU as the reference model writes it, the decoder head over given taps, the
state-dict recipes such tests load, and the engine's tensor layouts built with torch.

Nothing in the references knows how the engine folds, pads, splits or transforms anything: the conv is
``F.conv3d`` in float64 on the raw weights, BatchNorm is applied as written. The one exception is marked as
such: the emulations of two kernel families' designed arithmetic (``winograd_emulation``,
``split2_emulation``), which say what rounding a design costs on a case and never serve as a reference.
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


def _as_tensor(v):
    return v.clone() if torch.is_tensor(v) else torch.tensor(v)


def pow2(k):
    """2^k of an integer tensor, in float64 (exact for |k| <= 1022)."""
    return torch.ldexp(torch.ones(k.shape, dtype=torch.float64), k.to(torch.int32))


def rescale_state_dict(sd, K, seed):
    """A state dict that computes the same function as `sd` with every channel of every activation moved by
    its own power of two: channel c of a producer (a BatchNorm's gamma and beta) times 2^k(c), the input-channel
    columns c of every conv that reads it divided by 2^k(c), k uniform in [-K, K] and not constant. Every
    product x_c * w_c is then exactly the one `sd` gives (times the 2^j of the output channel it is summed
    into), so, while nothing overflows or underflows, an implementation whose steps commute with powers of
    two (sums, products, roundings to a binary format, ReLU, linear transforms with fixed coefficients)
    returns the same bits: motion unchanged, class j of the seg logits times 2^(out["segmentation_head"][j]).

    Sets: 25 inner ones (the stem's BatchNorm and, per block, conv1.0.1, conv1.1 and conv2.0.1, each read by
    one conv); one per residual stream (layer1: stem.4 and both blocks' conv2.1; layer L > 1: the blocks'
    conv2.1 and the downsample's BatchNorm), read by the layer's and the next layer's convs and by the
    layer's columns of comb_1_layer; comb_batch_norm_1 and comb_batch_norm_2 in the head; the clip's three
    colour channels (stem.0's columns; the caller multiplies the clip by 2^clip); the seg head's two classes
    (weight and bias times 2^j).

    Returns (rescaled state dict of float32 tensors, exps) with exps = {"clip": k(3), "out": {BatchNorm or
    "segmentation_head": k per output channel}, "in": {conv (state-dict prefix): k per input channel}}; the
    conv that a BatchNorm follows has exps["out"][that BatchNorm] on its output channels."""
    gen = torch.Generator().manual_seed(seed)
    out = {k: _as_tensor(v) for k, v in sd.items()}
    exps = {"out": {}, "in": {}}
    R = "r2plus1d_model."

    def draw(c):
        while True:
            k = torch.randint(-K, K + 1, (c,), generator=gen)
            if int(k.min()) != int(k.max()):
                return k

    def mul(name, k, dim):
        v = out[name]
        shape = [1] * v.dim()
        shape[dim] = -1
        out[name] = (v.double() * pow2(k).view(shape)).to(v.dtype)

    def produce(bn, k):
        assert bn not in exps["out"], bn
        exps["out"][bn] = k
        mul(bn + ".weight", k, 0)
        mul(bn + ".bias", k, 0)

    def consume(conv, k, col0=0):
        w = out[conv + ".weight"]
        cur = exps["in"].setdefault(conv, torch.zeros(w.shape[1], dtype=torch.int64))
        assert not bool(cur[col0:col0 + k.numel()].any()), conv  # every column belongs to one set
        cur[col0:col0 + k.numel()] = k
        full = torch.zeros(w.shape[1], dtype=torch.int64)
        full[col0:col0 + k.numel()] = -k
        mul(conv + ".weight", full, 1)

    def pair(bn, conv):
        k = draw(out[bn + ".weight"].numel())
        produce(bn, k)
        consume(conv, k)

    pair(R + "stem.1", R + "stem.3")
    for li in range(1, 5):
        for b in range(2):
            pre = f"{R}layer{li}.{b}."
            pair(pre + "conv1.0.1", pre + "conv1.0.3")
            pair(pre + "conv1.1", pre + "conv2.0.0")
            pair(pre + "conv2.0.1", pre + "conv2.0.3")
    col0 = {1: (0, 64), 2: (128,), 3: (256,), 4: (512,)}
    for li in range(1, 5):
        pre = f"{R}layer{li}."
        k = draw(out[pre + "1.conv2.1.weight"].numel())
        for bn in ((R + "stem.4",) if li == 1 else (pre + "0.downsample.1",)) + (pre + "0.conv2.1", pre + "1.conv2.1"):
            produce(bn, k)
        readers = [pre + "1.conv1.0.0"] + ([pre + "0.conv1.0.0"] if li == 1 else [])
        if li < 4:
            readers += [f"{R}layer{li + 1}.0.conv1.0.0", f"{R}layer{li + 1}.0.downsample.0"]
        for conv in readers:
            consume(conv, k)
        for c0 in col0[li]:
            consume("comb_1_layer", k, c0)
    k = draw(64)
    produce("comb_batch_norm_1", k)
    consume("comb_2_layer", k)
    k = draw(64)
    produce("comb_batch_norm_2", k)
    consume("segmentation_head", k)
    consume("motion_head", k)
    exps["clip"] = draw(3)
    consume(R + "stem.0", exps["clip"])
    j = draw(2)
    exps["out"]["segmentation_head"] = j
    mul("segmentation_head.weight", j, 0)
    mul("segmentation_head.bias", j, 0)
    return out, exps


def spread_unit(shape, gen, spread=12, per=2, dtype=torch.float64):
    """signed_unit times 2^a, a an integer uniform in [-spread, spread] drawn once per index of the first `per`
    dimensions (per = 2: one exponent per (n, c) or (o, c), constant over the rest)."""
    a = torch.randint(-spread, spread + 1, tuple(shape[:per]) + (1,) * (len(shape) - per), generator=gen)
    return (signed_unit(shape, gen, torch.float64) * pow2(a)).to(dtype)


def spread_state_dict(param_table, seed=0, spread=12):
    """float_state_dict with the operands of a real checkpoint's shape: conv weights signed_unit * 2^b(o, c),
    b uniform in [-spread, spread]; BatchNorm gamma with a random sign, two channels of every BatchNorm with
    gamma = 0 (dead: the output is beta) and two others with running_var = 0 (scale gamma / sqrt(eps))."""
    gen = torch.Generator().manual_seed(seed)
    sd = float_state_dict(param_table, seed)
    for name, shape in param_table:
        if len(shape) >= 2:
            sd[name] = spread_unit(shape, gen, spread, 2, torch.float32)
    for name, shape in param_table:
        if name.endswith("running_var"):
            pre = name[: -len(".running_var")]
            c = shape[0]
            sd[pre + ".weight"] = sd[pre + ".weight"] * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1).float()
            dead = torch.randperm(c, generator=gen)[:4]
            sd[pre + ".weight"][dead[:2]] = 0.0
            sd[name][dead[2:]] = 0.0
    return sd


def spread_draw(gen, spread=12, zeros=0.4, per_element=False):
    """draw(shape) for (N, C, T, H, W) activations: signed_unit * 2^a(n, c) (per_element: a per element), `zeros`
    of the elements exactly 0 and two whole channels (of every clip; one of the clip's three colours) 0, as
    after a ReLU."""
    def draw(shape):
        x = spread_unit(shape, gen, spread, len(shape) if per_element else 2)
        x = x * (torch.rand(shape, generator=gen, dtype=torch.float64) >= zeros)
        x[:, torch.randperm(shape[1], generator=gen)[:2 if shape[1] > 3 else 1]] = 0.0
        return x
    return draw


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


# ---- designed arithmetic of kernel families, emulated --------------------------------------------------
# What a kernel family is designed to compute, step by step, from the operands alone (never from a kernel's
# output): the error of these against the float64 reference is the rounding the design itself costs on a case.
# Lavin & Gray's F(2,3) and F(4,3) (points 0, +-1, +-2, infinity) matrices B^T, G, A^T.
WINOGRAD = {
    2: ([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
        [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]],
        [[1, 1, 1, 0], [0, 1, -1, -1]]),
    4: ([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
         [0, 4, 0, -5, 0, 1]],
        [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
         [0, 0, 1]],
        [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]),
}


def _windows(x, dim, m):
    """Windows of m + 2 at stride m along `dim` of x zero-padded by one in front and up to whole tiles behind:
    `dim` becomes the tile index, the window a new last dimension."""
    x = x.movedim(dim, -1)
    n = x.shape[-1]
    x = F.pad(x, (1, -(-n // m) * m + 1 - n)).unfold(-1, m + 2, m)
    return x.movedim(-2, dim)


def winograd_emulation(x, wf, shift, res, m):
    """The fused Winograd kernels' design for a stride-1 1x3x3 (F(m x m, 3x3), m = 2 or 4) or 3x1x1 (F(m, 3) in
    time) conv, in its own precisions: U = G g G^T in double from the folded double weights, rounded to fp32;
    V = B^T d B in fp32 (each one-sided transform rounded once); M = sum_c U V as exact products added to an fp32
    accumulator four input channels at a time (one fp32 MFMA step); Y = A^T M A likewise, + shift, + res in
    fp32. x (N,C,T,H,W), wf (O,C,kt,kh,kw), res float64 holding fp32 values; returns (N,O,T,H,W) float64,
    pre-activation."""
    BT, G, AT = (torch.tensor(a, dtype=torch.float64) for a in WINOGRAD[m])
    n, c, t, h, w = x.shape
    spatial = wf.shape[2] == 1
    # every step in float64 (the few-term sums with small integer coefficients are exact there) and rounded to
    # fp32 once, so the result does not depend on the host's float32 library
    f32 = lambda a: a.float().double()
    if spatial:
        d = _windows(_windows(x, 4, m), 3, m)                         # (N,C,T,th,tw,a_w,a_h)
        v = f32(torch.einsum("ia,nctpqba->nctpqib", BT, d))
        v = f32(torch.einsum("jb,nctpqib->nctpqij", BT, v))           # (N,C,T,th,tw,i,j)
        u = f32(torch.einsum("ia,ocab,jb->ocij", G, wf[:, :, 0], G))
        mm = "ocij,nctpqij->ntpqoij"
    else:
        d = _windows(x, 2, m)                                         # (N,C,tt,H,W,a)
        v = f32(torch.einsum("ia,ncphwa->ncphwi", BT, d))
        u = f32(torch.einsum("ia,oca->oci", G, wf[:, :, :, 0, 0]))
        mm = "oci,ncphwi->nphwoi"
    acc = 0.0
    for k in range(0, c, 4):
        acc = f32(acc + torch.einsum(mm, u[:, k:k + 4], v[:, k:k + 4]))
    if spatial:
        y = f32(torch.einsum("ri,ntpqoij->ntpqorj", AT, acc))
        y = f32(torch.einsum("sj,ntpqorj->ntpqors", AT, y))            # (N,T,th,tw,O,m,m)
        y = y.permute(0, 4, 1, 2, 5, 3, 6).reshape(n, -1, t, y.shape[2] * m, y.shape[3] * m)[..., :h, :w]
    else:
        y = f32(torch.einsum("ri,nphwoi->nphwor", AT, acc))            # (N,tt,H,W,O,m)
        y = y.permute(0, 4, 1, 5, 2, 3).reshape(n, -1, y.shape[1] * m, h, w)[:, :, :t]
    if shift is not None:
        y = f32(y + shift.view(1, -1, 1, 1, 1))
    if res is not None:
        y = f32(y + res)
    return y


def split2_emulation(x, wf, shift, stride, padding):
    """conv_stem_bf16's design: x and the folded fp32 weight each as hi + lo in bf16 (lo = bf16 of the
    remainder), the products hi.hi + hi.lo + lo.hi (lo.lo dropped), here summed exactly; + shift."""
    xh, wh = to_bf16(x), to_bf16(wf)
    xl, wl = to_bf16(x - xh), to_bf16(wf - wh)
    y = sum(F.conv3d(a, b, None, stride, padding) for a, b in ((xh, wh), (xh, wl), (xl, wh)))
    return y + shift.view(1, -1, 1, 1, 1)


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
