"""The engine across fp32's dynamic range (oracle/layer_ref.py: rescale_state_dict, spread_state_dict).

Every float operand of the other layer and forward tests lies in one binade. Here:
 (3a) whole forwards under the rescaling recipe: channel c of every BatchNorm, of the clip and of the seg head
      times 2^k(c), k uniform in [-K, K], compensated in the consumers' columns. Every product is unchanged
      (tests/test_dynamic_range_host.py: the CPU oracle returns the same bits), so motion and seg / 2^j must be
      bit-identical to the base weights', for both engine dtypes, K = 8 and 30, and every kernel variant;
 (3b) every case of test_layers_gpu.CASES and the decoder alone, base against rescaled (K = 30), bit for bit:
      localises a failure of (3a) to a kernel, and needs no float64 reference;
 (3c) operands spread over 2^+-12 independently (products of one sum span many binades), with exact zeros, dead
      BatchNorm channels and negative gammas, against the float64 reference under the families' unchanged bars
      (the Winograd families and conv_stem_bf16: or 4 x the error of their designed arithmetic, emulated);
 (4)  the recipe at K = 60 and 100, beyond the supported range: runs, reports, asserts nothing about the bits.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import layer_ref as LR
from tests import test_layers_gpu as TL

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 8, 32, 48), (2, 3, 16, 64, 96), (1, 3, 32, 112, 112)]
# every single variant bit the cases of test_layers_gpu.py set, per engine dtype
VARIANTS = {d: sorted({f for c in TL.CASES if c["dtype"] == d for f in c["flags"]} |
                      {f for dd, fl in TL.DEC_ENGINES if dd == d for f in fl}) for d in ("fp32", "bf16")}


def shape_id(s):
    return "x".join(map(str, s))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def times_pow2(t, k, dim=-1):
    """t * 2^k along dim (k shorter than the dimension: the padding channels stay as they are), exactly, in
    t's dtype."""
    f = torch.zeros(t.shape[dim], dtype=torch.int64)
    f[:k.numel()] = k
    shape = [1] * t.dim()
    shape[dim] = -1
    return (t.double() * LR.pow2(f).view(shape).to(t.device)).to(t.dtype)


# ---- (3a) whole forwards ------------------------------------------------------------------------------
_MODELS = {}


def forward_model(dtype, recipe, K):
    """(model, exps) of `recipe` after rescale_state_dict(K) (K = 0: the recipe itself, exps None)."""
    key = (dtype, recipe, K)
    if key not in _MODELS:
        from clasfv_amd.model import R2plus1D_18_MotionNet
        m = R2plus1D_18_MotionNet(pretrained=False, dtype=dtype, weights=recipe)
        exps = None
        if K:
            sd, exps = LR.rescale_state_dict(m.state_dict(), K, seed=1000 + K)
            m.load_state_dict(sd)
        _MODELS[key] = (m, exps)
    return _MODELS[key]


def clip(shape):
    return torch.from_numpy(np.random.default_rng(sum(shape)).uniform(0, 1, shape).astype(np.float32))


def rescaled_forward_pair(dtype, recipe, K, shape, variants=()):
    """(seg, mot) of the base weights and (seg / 2^j, mot) of the rescaled ones on the rescaled clip."""
    (base, _), (resc, exps) = forward_model(dtype, recipe, 0), forward_model(dtype, recipe, K)
    x = clip(shape)
    x2 = times_pow2(x, exps["clip"], 1)
    assert "no_winograd" not in variants  # the one variant that changes the weight images: it would need a reload
    for m in (base, resc):
        m.engine.set_variants(*variants)
    try:
        s0, m0 = TL.on_device(lambda: base(x))
        s1, m1 = TL.on_device(lambda: resc(x2))
        torch.cuda.synchronize()
    finally:
        for m in (base, resc):
            m.engine.set_variants()
    return (s0, m0), (times_pow2(s1, -exps["out"]["segmentation_head"], 1), m1)


def assert_same_bits(a, b, what):
    bad = bits(a) != bits(b)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} values differ, max |diff| " \
                                f"{float((a.double() - b.double()).abs().max()):.3e} (max |value| {float(a.abs().max()):.3e})"


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("recipe,K", [("random", 8), ("random", 30), ("deep", 30)], ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_is_exact_under_rescaling(dtype, recipe, K, shape):
    """Motion and seg / 2^j of the rescaled weights on the rescaled clip are the base weights' bits."""
    (s0, m0), (s1, m1) = rescaled_forward_pair(dtype, recipe, K, shape)
    assert bool(torch.isfinite(s0).all()) and float(s0.abs().max()) > 0
    assert_same_bits(m0, m1, "motion")
    assert_same_bits(s0, s1, "seg")


@pytest.mark.parametrize("dtype,variant", [(d, v) for d in ("fp32", "bf16") for v in VARIANTS[d]], ids=lambda v: str(v))
def test_forward_is_exact_under_rescaling_with_each_variant(dtype, variant):
    """The same at the smallest shape and K = 30 with one variant bit set: the kernels behind the product's."""
    (s0, m0), (s1, m1) = rescaled_forward_pair(dtype, "random", 30, SHAPES[0], (variant,))
    assert_same_bits(m0, m1, "motion")
    assert_same_bits(s0, s1, "seg")


# ---- (3b) every kernel alone --------------------------------------------------------------------------
def case_exponents(resc, c):
    """(input-channel exponents, output-channel exponents) of a case's conv in the rescaled net."""
    e = resc.by_name[c["layer"]]
    if e["tap"] >= 0:
        o0 = TL.COL0[c["layer"]]
        return resc.exps["in"]["comb_1_layer"][o0:o0 + e["cin"] + e["cin2"]], resc.exps["out"]["comb_batch_norm_1"]
    return resc.exps["in"][e["prefix"]], resc.exps["out"][e["bn"]]


def rescaled_case(resc, c, b):
    """The inputs of build_case's b for the rescaled net: x (and x2) times the conv's input-channel 2^k, res
    times its output-channel 2^j, between guard bands of their own."""
    e = b["e"]
    kin, kout = case_exponents(resc, c)
    dev = resc.engine.device
    x = b["x"]
    if c["x_c8"]:  # [cin_p / 8][voxels][8]: channel = 8 * block + lane
        k = torch.zeros(e["cin_p"], dtype=torch.int64)
        k[:e["cin"]] = kin
        x = (x.double() * LR.pow2(k).view(-1, 1, 8).to(dev)).to(x.dtype)
    else:
        x = times_pow2(x, kin[:e["cin"]])
    x, rec = TL.guarded_input(x, dev)
    out = dict(b, x=x, inputs=[rec])
    if b["x2"] is not None:
        out["x2"], rec = TL.guarded_input(times_pow2(b["x2"], kin[e["cin"]:]), dev)
        out["inputs"].append(rec)
    if b["res"] is not None:
        out["res"], rec = TL.guarded_input(times_pow2(b["res"], kout), dev)
        out["inputs"].append(rec)
    return out


def rescaled_conv_mismatch(base, resc, c):
    """Runs the case on both nets (launch() asserts the memory discipline of check (c) on each run); returns
    a description of the first ReLU setting whose outputs are not base * 2^j bit for bit, or None."""
    b0 = TL.build_case(base, c, reference=False)
    b1 = rescaled_case(resc, c, b0)
    _, kout = case_exponents(resc, c)
    for relu in c["relu"]:
        _, _, full0 = TL.launch(base, c, b0, relu)
        _, _, full1 = TL.launch(resc, c, b1, relu)
        assert bool(torch.isfinite(full0.float()).all())
        want = times_pow2(full0, kout)
        bad = bits(want) != bits(full1)
        if bool(bad.any()):
            rel = ((full1.double() - want.double()).abs() / want.double().abs().clamp_min(1e-300))[bad]
            return f"relu={relu}: {int(bad.sum())} of {bad.numel()} outputs differ from base * 2^j, " \
                   f"max relative difference {float(rel.max()):.3e}"
    return None


@pytest.mark.parametrize("c", TL.CASES, ids=TL.case_id)
def test_conv_alone_is_exact_under_rescaling(c):
    """The case on the float recipe, and on the same recipe rescaled (K = 30) with x, x2 times the conv's
    input-channel 2^k and res times its output-channel 2^j: the second output is the first times 2^j, bit for
    bit, padded channels +0, guards and inputs intact."""
    bad = rescaled_conv_mismatch(TL.net(c["dtype"], "float"), TL.net(c["dtype"], "rescaled"), c)
    assert bad is None, bad


def rescaled_decoder_pair(base, resc, nthw, flags, seed_k=0):
    n, t, h, w = nthw
    gen = torch.Generator().manual_seed(t * 1000 + h * 10 + w + seed_k)
    taps = [LR.to_channels_last(LR.signed_unit((n, 64) + s, gen, torch.float32), 64, torch.float32)
            for s in LR.tap_shapes(t, h, w)]
    out = []
    for nt, k in ((base, None), (resc, resc.exps["out"]["comb_batch_norm_1"])):
        dev = nt.engine.device
        taps_dev, records = zip(*[TL.guarded_input(p if k is None else times_pow2(p, k), dev) for p in taps])
        _, sbits, seg = TL.guarded(n * 2 * t * h * w, torch.float32, dev)
        _, mbits, mot = TL.guarded(n * 4 * t * h * w, torch.float32, dev)
        old = nt.engine.set_variants(*flags)
        try:
            TL.on_device(lambda: (nt.engine.run_decoder(taps_dev, nthw, seg, mot), torch.cuda.synchronize()))
        finally:
            nt.engine.set_variants(*old)
        assert TL.inputs_intact(records), "a decoder tap or its guard bands were written"
        assert TL.guards_intact(sbits) and TL.guards_intact(mbits), "write outside seg / motion"
        assert bool((sbits[TL.GUARD:-TL.GUARD] != -1).all()) and bool((mbits[TL.GUARD:-TL.GUARD] != -1).all())
        seg = seg.reshape(n, 2, t, h, w)
        if k is not None:
            seg = times_pow2(seg, -resc.exps["out"]["segmentation_head"], 1)
        out.append((seg, mot.clone()))
    return out


@pytest.mark.parametrize("dtype,flags", TL.DEC_ENGINES, ids=lambda v: v if isinstance(v, str) else "-".join(v) or "product")
@pytest.mark.parametrize("nthw", TL.DEC_SHAPES, ids=shape_id)
def test_decoder_alone_is_exact_under_rescaling(nthw, dtype, flags):
    """clasfv_run_decoder on taps times comb_batch_norm_1's 2^k with the rescaled head: the same motion and
    seg / 2^j, bit for bit."""
    (s0, m0), (s1, m1) = rescaled_decoder_pair(TL.net(dtype, "float"), TL.net(dtype, "rescaled"), nthw, flags)
    assert_same_bits(m0, m1, "motion")
    assert_same_bits(s0, s1, "seg")


# ---- (3c) spread operands against float64 -------------------------------------------------------------
DIRECT_FAMILIES = ("x3", "f32", "bf16", "stem_bf16")


def spread_cases():
    """One case per (kernel, dtype) of FAMILY: the smallest nthw CASES lists for the kernel, in its plain form and,
    where CASES has the kernel with them, with a residual and with the blocked layouts; the direct-form
    families a second time with an exponent per element."""
    out = []
    for kernel, dtype in TL.FAMILY:
        mine = [c for c in TL.CASES if c["kernel"] == kernel and c["dtype"] == dtype]
        size = lambda c: c["nthw"][0] * c["nthw"][1] * c["nthw"][2] * c["nthw"][3]
        picked = []
        plain = {"res": False, "x_c8": False, "y_c8": False}
        for form in (plain, {"res": True}, {"x_c8": True}, {"y_c8": True}):
            fit = [c for c in mine if all(c[k] == v for k, v in form.items())]
            if fit and not any(c in picked for c in fit):
                picked.append(min(fit, key=size))
        for c in picked:
            out.append((c, False))
            if TL.FAMILY[(kernel, dtype)] in DIRECT_FAMILIES and c is picked[0]:
                out.append((c, True))
    return out


def measure(y, ref, den, bf_out):
    """Check (b)'s e of an output against the reference: max |y - ref| / den, a bf16 output allowed one bf16 ulp
    of |ref|; an output with den == 0 (nothing was added to it) must be exactly 0."""
    err = (y - ref).abs()
    if bf_out:
        err = (err - LR.bf16_ulp(ref)).clamp_min(0)
    assert bool((err[den == 0] == 0).all()), "an output with nothing added to it is not exactly 0"
    return float((err / den.clamp_min(1e-300)).max())


def designed_error(c, b):
    """e of the family's designed arithmetic, emulated on the CPU from the case's operands alone (oracle/
    layer_ref.py: winograd_emulation, split2_emulation), over the case's ReLU settings; None for the families
    whose BARS entry holds on the spread cases as it is."""
    e, fam = b["e"], TL.FAMILY[(c["kernel"], c["dtype"])]
    if fam in ("wino4", "wino2", "winot"):
        y = LR.winograd_emulation(b["x64"], b["wf"], b["shift"], b["res64"], 2 if fam == "wino2" else 4)
    elif fam == "stem_bf16":
        y = LR.split2_emulation(b["x64"], b["wf"], b["shift"], e["stride"], e["padding"])
    else:
        return None
    bf_out = e["out_dtype"] == torch.bfloat16
    worst = 0.0
    for relu in c["relu"]:
        out, ref = (F.relu(y), F.relu(b["y64"])) if relu else (y, b["y64"])
        worst = max(worst, measure(LR.to_bf16(out) if bf_out else out, ref, b["den"], bf_out))
    return worst


def spread_id(v):
    return TL.case_id(v[0]) + ("-per_element" if v[1] else "")


@pytest.mark.parametrize("case", spread_cases(), ids=spread_id)
def test_conv_spread_operands_vs_float64(case):
    """Check (b) of test_layers_gpu.py on the spread recipe: activations signed_unit * 2^a(n, c) (a second draw of
    the direct-form kernels: a per element), 40 % of them 0 and two whole channels 0, weights signed_unit *
    2^b(o, c), a, b uniform in [-12, 12], gammas of either sign, two dead channels (gamma = 0) and two of
    running_var = 0 per BatchNorm. e = max |y - y64| / (conv3d(|x|, |w_f|) + |b_f| + |res|) stays under the family's bar
    of BARS, unchanged, for the direct-form fp32 and the bf16 families: every product's error is relative to
    itself, so e cannot grow when the products are rescaled. Dead channels come out as exactly beta (+ res),
    rounded once. launch() asserts the checks of (c).

    The Winograd families and conv_stem_bf16 take max(BARS entry, 4 x the e of their designed arithmetic emulated
    on the same case) (designed_error: from the operands alone; 4 x is BARS' own margin for summation order).
    Their design's rounding is not relative to an output's own products: a transform spreads the rounding of a
    tile's large elements over all its outputs, among them outputs whose own taps of the dominant channel are
    the exact zeros of the draw (all 3 taps of a 3x1x1 conv: 6 % of the outputs) and whose denominator
    therefore comes from channels 2^-12 below; the direct sums of the other cases average this over hundreds of
    comparable channels. Measured on the MI355X, kernel against emulation (profiles/dynamic_range_mi355x.txt):
    wino4 7.5e-5 / 1.0e-4, wino2 8.0e-7 / 5.5e-7, winot 5.0e-4 / 4.1e-4 (stem.3: 45 input channels), and
    conv_stem_bf16 with an exponent per element 3.570e-6 / 3.570e-6 (its dropped lo.lo products, 2^-16 of a
    product each, next to nothing else in the sum): the kernels compute what they were designed to."""
    c, per_element = case
    nt = TL.net(c["dtype"], "spread")
    b = TL.build_case(nt, c, per_element=per_element)
    e = b["e"]
    fam = TL.FAMILY[(c["kernel"], c["dtype"])]
    bf_out = e["out_dtype"] == torch.bfloat16
    chans = b["chans"] if b["chans"] is not None else torch.arange(e["cout"])
    gamma = nt.sd[("comb_batch_norm_1" if e["tap"] >= 0 else e["bn"]) + ".weight"][chans]
    dead = gamma == 0
    assert int((nt.sd[("comb_batch_norm_1" if e["tap"] >= 0 else e["bn"]) + ".weight"] == 0).sum()) == 2
    if c["relu"] == (True,):  # compared after ReLU only: the case must not compare zeros
        assert float((b["y64"] > 0).double().mean()) >= 0.4, "ReLU-only kernel: too few positive reference outputs"
    worst = 0.0
    for relu in c["relu"]:
        y, _, full = TL.launch(nt, c, b, relu)
        assert bool(torch.isfinite(y).all())
        ref = F.relu(b["y64"]) if relu else b["y64"]
        got = y[:, chans] if b["chans"] is not None else y
        worst = max(worst, measure(got, ref, b["den"], bf_out))
        if bool(dead.any()):
            want = ref[:, dead].float()
            want = want.bfloat16().double() if bf_out else want.double()
            assert torch.equal(got[:, dead], want), "a gamma = 0 channel is not exactly beta (+ res)"
        if c["res"]:
            _, _, full2 = TL.launch(nt, c, b, relu, alias=True)
            assert torch.equal(bits(full2), bits(full)), "res aliasing y changes the result"
    bar, emul = TL.BARS[fam], designed_error(c, b)
    if emul is not None:
        bar = max(bar, 4 * emul)
    print(f"SPREAD_ERR {fam} {spread_id(case)} e={worst:.3e} bar={bar:.3e} family_bar={TL.BARS[fam]:.3e} "
          f"emulated={'n/a' if emul is None else format(emul, '.3e')} denmax={float(b['den'].max()):.4e} "
          f"positive={float((b['y64'] > 0).double().mean()):.3f}")
    assert worst <= bar, f"e = {worst:.3e} above the {fam} bar {bar:.3e}"


def test_spread_cases_reach_every_kernel_and_form():
    cases = spread_cases()
    assert {(c["kernel"], c["dtype"]) for c, _ in cases} == set(TL.FAMILY)
    for form in ("res", "x_c8", "y_c8"):
        assert {c["kernel"] for c in TL.CASES if c[form]} == {c["kernel"] for c, _ in cases if c[form]}
    assert {TL.FAMILY[(c["kernel"], c["dtype"])] for c, p in cases if p} == set(DIRECT_FAMILIES)


# ---- (4) beyond the supported range -------------------------------------------------------------------
@pytest.mark.parametrize("K", [60, 100])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_beyond_the_tested_range_runs(dtype, K):
    """Exponents in [-K, K] for K = 60 and 100: folded weights w * 2^(j - k) and the small pieces of small
    activations leave fp32's / bf16's normal range, so the bits may differ ("Dynamic range";
    profiles/dynamic_range_mi355x.txt). These are ordinary finite inputs: the forward runs and writes every
    output; what it writes is reported, not asserted."""
    (s0, m0), (s1, m1) = rescaled_forward_pair(dtype, "random", K, SHAPES[0])
    same = lambda a, b: int((bits(a) != bits(b)).sum())
    far = lambda a, b: float(torch.nan_to_num((a.double() - b.double()).abs(), nan=0.0, posinf=0.0).max())
    print(f"DYNRANGE {dtype} K={K} seg differs in {same(s0, s1)} of {s0.numel()} (max finite |diff| {far(s0, s1):.3e}) "
          f"motion in {same(m0, m1)} of {m0.numel()} (max |diff| {far(m0, m1):.3e}) "
          f"finite seg={bool(torch.isfinite(s1).all())} motion={bool(torch.isfinite(m1).all())}")
    assert bool(torch.isfinite(s0).all()) and bool(torch.isfinite(m0).all())
