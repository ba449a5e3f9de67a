"""The forward's launch plan, audited on the host (no GPU, no oracle binaries).

clasfv_forward_plan records what clasfv_forward issues -- every launch with the memory it reads and writes,
the side stream's fork and join events, each sub-batch's arena layout -- from the forward's own walk.
tests/plan_audit.py checks the arena's contract on it ("The arena's contract": A layout,
B footprints, C hazards, D definition before use, E the batch does not choose the arithmetic, F sub-batch
sizes). First the checker is shown to fail: hand-written plans with one seeded defect each. Then the real
plans, both dtypes: the four shapes of tests/test_engine_state_gpu.py, the product batches, sub-batched calls,
and every single variant bit at two shapes.

What the audit found when it first ran, kept as test_which_convs_split: at the product clip the per-clip
split-K rule also selected layer4's three 7x7 spatial convs on conv_dma_x3, which the forward never gave a
scratch (only a conv that reads MID has one), so they asked for four partial sums and silently ran unsplit,
while clasfv_run_conv with a scratch ran them split. The outcome never depended on N, so no bits were wrong;
the engine now says what it does: a conv that is offered no scratch asks for no split, every conv that reads
MID is offered one whatever is left of it, and a scratch too small shows as asked > granted (check E).
"""
import copy

import pytest

from oracle import layer_ref as LR
from tests import plan_audit as PA

DTYPES = ("fp32", "bf16")
SMALL, RAGGED, FIVE, CLIP = (1, 8, 16, 32), (2, 16, 64, 48), (3, 24, 80, 112), (1, 32, 112, 112)
SHAPES = (SMALL, RAGGED, FIVE, CLIP, (12, 32, 112, 112), (1, 64, 224, 224))


def shape_id(s):
    return "x".join(map(str, s))


# ---- the checker's self-test ----------------------------------------------------------------------------------
def rng(buffer, role, write, offset, nbytes):
    return {"buffer": buffer, "role": role, "write": write, "offset": offset, "bytes": nbytes}


def launch(kind, stream=0, conv=-1, kernel="", ranges=(), asked=1, granted=1, res=0):
    return {"sub_batch": 0, "stream": stream, "kind": kind, "conv": conv, "kernel": kernel, "split_asked": asked,
            "split_granted": granted, "x_c8": 0, "y_c8": 0, "relu": 1, "has_res": res, "x_elem": 4, "y_elem": 4,
            "ranges": list(ranges)}


XIN, F0, F1, SCR, P, IDX = range(6)
OFF = {XIN: (0, 1000), F0: (1024, 960), F1: (2048, 512), SCR: (2560, 512), P: (3072, 256), IDX: (3328, 128)}
C0, C2, C1, SUM, JOIN, DEC = 1, 3, 4, 5, 6, 8  # positions in clean_plan()'s launches


def whole(b, role, write):
    return rng(b, role, write, *OFF[b])


def clean_plan():
    """pack -> c0 -> fork, c2 on the side stream | c1 with a split and its sum -> join -> decoder."""
    buffers = [{"sub_batch": 0, "clips": 1, "id": b, "name": n, "offset": OFF[b][0], "bytes": OFF[b][1], "total": 3584}
               for b, n in enumerate(("XIN", "F0", "F1", "SCR", "P", "IDX"))]
    launches = [
        launch("pack", kernel="pack_input_kernel", ranges=[rng(-1, "x", False, 0, 750), whole(XIN, "y", True)]),
        launch("conv", conv=0, kernel="k0", ranges=[whole(XIN, "x", False), whole(F0, "y", True)]),
        launch("fork", stream=1),
        launch("conv", stream=1, conv=2, kernel="k2", ranges=[whole(F0, "x", False), whole(P, "y", True)]),
        launch("conv", conv=1, kernel="k1", asked=2, granted=2,
               ranges=[whole(F0, "x", False), whole(XIN, "x2", False), whole(SCR, "part", True)]),
        launch("split_sum", conv=1, kernel="split_sum_kernel", asked=2, granted=2,
               ranges=[whole(SCR, "part", False), whole(F1, "y", True)]),
        launch("join"),
        launch("dec_index", kernel="decoder_index_kernel", ranges=[whole(IDX, "idx", True)]),
        launch("decoder", kernel="decoder_kernel",
               ranges=[whole(P, "tap", False), whole(F1, "tap", False), whole(IDX, "idx", False),
                       rng(-2, "y", True, 0, 500), rng(-3, "y", True, 0, 1000)]),
    ]
    return {"buffers": buffers, "launches": launches}


def seeded(defect):
    p = clean_plan()
    ls = p["launches"]
    if defect == "a range past its buffer":          # c0 writes 40 bytes into the slack after F0
        ls[C0]["ranges"][1]["bytes"] = 1000
    elif defect == "two overlapping buffers":        # F0 grows into F1
        p["buffers"][F0]["bytes"] = 1100
    elif defect == "a side-stream write over a main-stream read":  # c2 also writes what c1 reads, no join between
        ls[C2]["ranges"].append(rng(XIN, "part", True, 0, 256))
    elif defect == "a read before any write":        # c1 reads F1, which only its own sum writes, later
        ls[C1]["ranges"][1] = rng(F1, "x2", False, 2048, 256)
    elif defect == "a granted split below the asked one":  # c1 unsplit: writes F1 itself, no sum
        ls[C1]["split_granted"] = 1
        ls[C1]["ranges"][2] = whole(F1, "y", True)
        del ls[SUM]
    elif defect == "a missing join before the decoder":
        del ls[JOIN]
    else:
        raise KeyError(defect)
    return p


SEEDS = {
    "a range past its buffer": {"range-outside-buffer"},
    "two overlapping buffers": {"buffers-overlap"},
    "a side-stream write over a main-stream read": {"race"},
    "a read before any write": {"read-of-unwritten"},
    "a granted split below the asked one": {"split-refused"},
    # the decoder's read of P is then both unordered with c2's write (C) and not defined before it (D)
    "a missing join before the decoder": {"race", "read-of-unwritten"},
}


def test_the_clean_hand_written_plan_has_no_violation():
    assert PA.audit(clean_plan()) == []
    assert PA.check_split_sums(clean_plan()) == []


@pytest.mark.parametrize("defect", sorted(SEEDS))
def test_the_checker_reports_exactly_the_seeded_defect(defect):
    got = PA.audit(seeded(defect))
    assert {v.what for v in got} == SEEDS[defect], got
    # one report per defect and check: nothing else in the plan is touched by it
    assert len(got) == len(SEEDS[defect]), got
    if defect == "a missing join before the decoder":
        assert sorted(v.check for v in got) == ["C", "D"]
        assert all("decoder" in v.detail for v in got)


def test_happens_before_is_only_what_the_events_order():
    ls = clean_plan()["launches"]
    ck = PA.clocks(ls)
    assert ck[2] is None and ck[JOIN] is None
    assert PA.before(ck[C0], ck[C2]) and not PA.before(ck[C2], ck[C0])      # the fork orders c2 after c0
    assert not PA.before(ck[C1], ck[C2]) and not PA.before(ck[C2], ck[C1])  # c1 was issued after the fork
    assert PA.before(ck[C2], ck[DEC]) and PA.before(ck[0], ck[DEC])         # the join, and transitivity
    # a second sub-batch: its pack is ordered after the first one's decoder and side stream through the join alone
    two = ls + [dict(l, sub_batch=1) for l in copy.deepcopy(ls)]
    ck2 = PA.clocks(two)
    assert PA.before(ck2[C2], ck2[len(ls)])
    without = [l for i, l in enumerate(two) if i != JOIN]
    ckw = PA.clocks(without)
    assert not PA.before(ckw[C2], ckw[len(ls) - 1]), "without the first join nothing orders the next pack after c2"


def test_batch_checks_report_a_changed_sequence_and_wrong_sub_batches():
    a, b = clean_plan(), clean_plan()
    assert PA.check_same_arithmetic(a, b) == []
    b["launches"][C1]["split_asked"] = 4
    assert [v.what for v in PA.check_same_arithmetic(a, b)] == ["sequence-depends-on-batch"]
    assert PA.check_sub_batches(a, 1, 1) == [] and PA.check_sub_batches(a, 1, 5) == []
    assert [v.what for v in PA.check_sub_batches(a, 2, 1)] == ["sub-batch-sizes"]
    no_sum = seeded("a granted split below the asked one")
    no_sum["launches"][C1]["split_granted"] = 2
    assert [v.what for v in PA.check_split_sums(no_sum)] == ["split-sum-placement"]


def test_written_elements_keeps_the_last_writer():
    p = clean_plan()
    p["launches"][SUM]["y_elem"] = 2
    p["launches"].insert(DEC, launch("conv", conv=3, kernel="k3", ranges=[rng(SCR, "y", True, 2560, 128)]))
    assert PA.written_elements(p) == [(0, 1000, 4), (1024, 1984, 4), (2048, 2560, 2), (2560, 2688, 4), (2688, 3072, 4),
                                      (3072, 3328, 4), (3328, 3456, None)]


# ---- real plans ----------------------------------------------------------------------------------------------------
_PLANS, _TABLES = {}, {}


def plan(dtype, n, thw, variants=()):
    from clasfv_amd.model import forward_plan
    key = (dtype, n, thw, tuple(variants))
    if key not in _PLANS:
        _PLANS[key] = forward_plan(n, *thw, dtype, variants)
    return _PLANS[key]


def table(dtype):
    from clasfv_amd.model import plan_conv_table
    if dtype not in _TABLES:
        _TABLES[dtype] = plan_conv_table(dtype)
    return _TABLES[dtype]


def max_clips(dtype, thw, variants=()):
    from clasfv_amd import _lib
    from clasfv_amd.model import variant_flags
    return _lib.load().clasfv_max_clips(*thw, _lib.DTYPES[dtype], variant_flags(variants))


def audit_real(dtype, n, thw, variants=()):
    """Every check on the plan of an n-clip call; returns the plan."""
    p = plan(dtype, n, thw, variants)
    mc = max_clips(dtype, thw, variants)
    assert mc >= 1
    sizes = [s[0] for s in PA.sub_batch_clips(p)]
    bad = (PA.audit(p) + PA.check_sub_batches(p, n, mc) + PA.check_split_sums(p)
           + PA.check_footprints(p, table(dtype), sizes, *thw, LR.out_dim, LR.tap_shapes)
           + PA.check_same_arithmetic(p, plan(dtype, 1, thw, variants)))
    assert bad == [], "\n".join(map(str, bad[:12]))
    assert sum(sizes) == n
    # the caller's tensors: each sub-batch reads and writes its own clips, and together they cover the call
    clip = thw[0] * thw[1] * thw[2] * 4
    for ext, per in ((-1, 3), (-2, 2), (-3, 4)):
        spans = [PA.span(r) for l in p["launches"] for r in l["ranges"] if r["buffer"] == ext]
        starts = [sum(sizes[:i]) * per * clip for i in range(len(sizes))]
        assert spans == [(a, a + m * per * clip) for a, m in zip(starts, sizes)], (ext, spans)
    return p


def test_the_conv_table_needs_no_handle_and_pads_as_the_kernels_need():
    for dtype in DTYPES:
        t = table(dtype)
        assert len(t) == 41 and [c["index"] for c in t] == list(range(41))
        step = 32 if dtype == "bf16" else 16
        assert t[0]["cin_p"] == 4 and all(c["cin_p"] % step == 0 for c in t[1:])
        assert all(c["cin_p"] >= c["cin"] and c["cout_p"] >= c["cout"] for c in t)
        assert [c["cin2"] for c in t[-4:]] == [64, 0, 0, 0] and all(c["cout_p"] == 64 for c in t[-4:])


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("dtype", DTYPES)
def test_product_plan(dtype, shape):
    p = audit_real(dtype, shape[0], shape[1:])
    kinds = [l["kind"] for l in p["launches"]]
    assert kinds[0] == "pack" and kinds[-2:] == ["dec_index", "decoder"]
    assert kinds.count("fork") == 3 and kinds.count("join") == 1
    assert [l["conv"] for l in p["launches"] if l["stream"] == 1 and l["kind"] == "conv"] == [37, 38, 39]
    # the device-less engine picks the kernels a finalized handle does: its stem took conv_stem_f32 on bf16
    # engines while the plan marked no bias present (tests/test_plan_gpu.py compares every launch with the log)
    assert p["launches"][1]["kernel"] == ("conv_stem_x3" if dtype == "fp32" else "conv_stem_bf16")


@pytest.mark.parametrize("thw,batches", [((32, 112, 112), (1, 2)), ((64, 224, 224), (1,))], ids=("32x112x112", "64x224x224"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_sub_batched_plan(dtype, thw, batches):
    mc = max_clips(dtype, thw)
    for k in batches:
        p = audit_real(dtype, k * mc + 1, thw)
        assert [s[0] for s in PA.sub_batch_clips(p)] == [mc] * k + [1]
        # the short last sub-batch has a layout of its own that fits the arena of the first
        totals = sorted({(b["sub_batch"], b["total"]) for b in p["buffers"]})
        assert totals[-1][1] < totals[0][1] and len({t for _, t in totals[:-1]}) == 1


def _variant_names():
    from clasfv_amd import _lib
    return sorted(_lib.VARIANTS)


@pytest.mark.parametrize("variant", _variant_names())
@pytest.mark.parametrize("shape", (RAGGED, CLIP), ids=shape_id)
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_variant_plan(dtype, shape, variant):
    audit_real(dtype, shape[0], shape[1:], (variant,))


# variant bit -> the kernels it switches off, by reported name: written here from include/clasfv.h's comments,
# not read from the engine's kernel table. A bit that is not listed switches no conv kernel off (it chooses a
# form inside a launcher, a layout, or the decoder's arithmetic).
_W4R, _W4W, _W4 = "conv_wino4r", "conv_wino4w", "conv_wino4"
SWITCHES_OFF = {
    "no_wino4r": {_W4R},
    "no_wino4w": {_W4R, _W4W},
    "no_wino4": {_W4R, _W4W, _W4},
    "no_wino_patch": {"conv_wino_q"},
    "no_stem_bf16": {"conv_stem_bf16"},
    "no_stem_x3": {"conv_stem_x3"},
    "no_proj_x3": {"conv_proj_x3"},
    "no_dma_x3": {"conv_proj_x3", "conv_dma_x3"},
    "no_patch32": {"conv_patch32_bf16"},
    "no_twalk": {"conv_twalk_bf16"},
    "no_patch_bf16": {"conv_patch32_bf16", "conv_twalk_bf16", "conv_patch_bf16"},
    "no_dma_w": {"conv_dma_w"},
    "no_dma_buf": {"conv_dma_w"},  # conv_dma_w has a buffer-offset form only: without it, conv_dma's pointer form
    "no_winograd": {_W4R, _W4W, _W4, "conv_wino_q", "conv_wino", "conv_winot"},
}
SWITCH_SHAPES = (SMALL, RAGGED, CLIP, (1, 64, 224, 224))
# (variants, the variants of the plan to compare with): every single bit against the product plan, and
# no_wino_patch below no_wino4, where conv_wino_q is what the F(4x4) kernels' convs fall to
SWITCH_CASES = [((v,), ()) for v in _variant_names()] + [(("no_wino4", "no_wino_patch"), ("no_wino4",))]


def conv_kernels(p):
    """conv index -> kernel name of a one-sub-batch plan."""
    return {l["conv"]: l["kernel"] for l in p["launches"] if l["kind"] == "conv"}


@pytest.mark.parametrize("variants,base", SWITCH_CASES, ids=lambda v: "+".join(v) or "product")
def test_a_variant_bit_removes_exactly_its_kernels(variants, base):
    """No conv of the variant's plan runs on a kernel the bit switches off, and every conv whose kernel differs
    from the base plan's ran on a switched-off kernel there: the bit moves its own kernels' convs and no other."""
    off = set().union(*(SWITCHES_OFF.get(v, set()) for v in set(variants) - set(base)))
    changed = {}
    for dtype in DTYPES:
        for shape in SWITCH_SHAPES:
            was, now = (conv_kernels(plan(dtype, shape[0], shape[1:], v)) for v in (base, variants))
            assert sorted(was) == sorted(now) == list(range(41))
            assert not off & set(now.values()), (dtype, shape, sorted(off & set(now.values())))
            moved = {i: (was[i], now[i]) for i in was if was[i] != now[i]}
            assert all(a in off for a, _ in moved.values()), (dtype, shape, moved)
            changed[dtype, shape] = moved
    if not off:
        return
    if variants == ("no_wino_patch",):  # the product's 1x3x3 convs are on the F(4x4) kernels: nothing to move
        assert not any(changed.values())
    else:
        assert any(changed.values()), "the bit switches kernels off that no plan here uses"
    if base:  # below no_wino4 the same bit moves conv_wino_q's convs to conv_wino, at every shape that has some
        for shape in (SMALL, RAGGED, CLIP):
            assert set(changed["fp32", shape].values()) == {("conv_wino_q", "conv_wino")}, shape


def test_which_convs_split():
    """The product clip: layer4's four temporal convs (they read MID, and MID has room past their input at
    every batch) split four ways; no other conv asks, the 7x7 spatial convs 30, 33 and 35 on conv_dma_x3
    included, which the per-clip rule would select but the forward has no scratch for. bf16 engines never
    split. no_split_k asks for none."""
    thw = CLIP[1:]
    mc = max_clips("fp32", thw)
    for n in (1, 2, 7, 12, 30, 32, mc):
        p = plan("fp32", n, thw)
        convs = [l for l in p["launches"] if l["kind"] == "conv"]
        assert {l["conv"]: l["split_granted"] for l in convs if l["split_asked"] > 1} == {29: 4, 31: 4, 34: 4, 36: 4}, n
        assert {l["kernel"] for l in convs if l["conv"] in (30, 33, 35)} == {"conv_dma_x3"}
        mid = next(b for b in p["buffers"] if b["name"] == "MID")
        for l in p["launches"]:
            for r in l["ranges"]:
                if r["role"] == "part":  # the sums live in MID, past the input of the conv that writes them
                    x = l["ranges"][0] if l["kind"] == "conv" else None
                    assert r["buffer"] == mid["id"] and (x is None or r["offset"] >= x["offset"] + x["bytes"])
    assert all(l["split_asked"] == 1 for l in plan("bf16", 12, thw)["launches"])
    assert all(l["split_asked"] == 1 for l in plan("fp32", 12, thw, ("no_split_k",))["launches"])


def test_plan_arguments():
    from clasfv_amd import _lib
    import ctypes
    lib = _lib.load()
    n = ctypes.c_int()
    none = (0, None, ctypes.byref(n), 0, None, None)
    assert lib.clasfv_forward_plan(0, 8, 16, 16, 0, 0, *none) == -1
    assert lib.clasfv_forward_plan(1, 12, 16, 16, 0, 0, *none) == -2
    assert lib.clasfv_forward_plan(1, 8, 16, 16, 2, 0, *none) == -1
    assert lib.clasfv_forward_plan(1, 8, 16, 16, 0, 1 << 17, *none) == -1
    assert lib.clasfv_forward_plan(1, 8, 16384, 16384, 0, 0, *none) == -2  # one clip no pass serves
    assert lib.clasfv_forward_plan(1, 8, 16, 16, 0, 0, *none) == 0 and n.value > 50
    small = (_lib.PlanLaunch * 4)()
    assert lib.clasfv_forward_plan(1, 8, 16, 16, 0, 0, 4, small, ctypes.byref(n), 0, None, None) == -1
    assert b"cap" in lib.clasfv_last_error()
    assert lib.clasfv_plan_conv_info(0, 41, None, None, None, None, None, None) == -1
    assert lib.clasfv_plan_conv_info(3, 0, None, None, None, None, None, None) == -1
    assert lib.clasfv_workspace_view(None, None, None, None) == -1
