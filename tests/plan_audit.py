"""A checker for the forward's launch plan (clasfv_forward_plan; DESIGN.md, "The arena's contract").

A plan is what clasfv_amd.model.forward_plan returns: {"launches": [...], "buffers": [...]}. Every function
here is plain Python over those dicts and returns a list of Violation; an empty list means the property
holds. Nothing here touches a device or the library, so hand-written plans can be audited as well
(tests/test_plan_host.py does, to show that each check can fail).

Happens-before, the only ordering the checks accept:
 * launches of one stream are ordered as issued;
 * a side-stream launch is after everything issued on the caller's stream before a fork that precedes it;
 * a launch on the caller's stream is after every side-stream launch issued before a join that precedes it;
 * nothing else orders two launches: a sub-batch is after the previous one only through these rules.
With two streams and monotone issue counters this relation is transitive as it stands.
"""
from collections import namedtuple

Violation = namedtuple("Violation", "check what detail")
MARKERS = ("fork", "join")
ALIGN = 256


# ---- intervals ----------------------------------------------------------------------------------------------
def merged(intervals):
    """Sorted, disjoint, non-empty union of half-open (a, b) intervals."""
    out = []
    for a, b in sorted(i for i in intervals if i[1] > i[0]):
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def uncovered(a, b, cover):
    """The parts of [a, b) outside `cover` (merged intervals)."""
    gaps = []
    for ca, cb in cover:
        if cb <= a:
            continue
        if ca >= b:
            break
        if ca > a:
            gaps.append((a, ca))
        a = max(a, cb)
    if a < b:
        gaps.append((a, b))
    return gaps


def span(r):
    return r["offset"], r["offset"] + r["bytes"]


def space(r):
    """Ranges can only overlap inside one address space: the arena, or one of the caller's tensors."""
    return "arena" if r["buffer"] >= 0 else r["buffer"]


def overlap(r, q):
    return space(r) == space(q) and r["offset"] < q["offset"] + q["bytes"] and q["offset"] < r["offset"] + r["bytes"]


def name_of(i, l):
    return f"#{i} sub {l['sub_batch']} {l['kind']} {l['kernel']} conv {l['conv']} stream {l['stream']}"


# ---- happens-before -----------------------------------------------------------------------------------------
def clocks(launches):
    """Per launch (None for a marker): (stream, own index on its stream, {stream: the largest index on that
    stream the launch is ordered after})."""
    issued = [0, 0]        # launches issued on each stream so far
    sees = [[0, 0], [0, 0]]  # sees[s][o]: what stream s is ordered after on stream o
    out = []
    for l in launches:
        if l["kind"] == "fork":    # the side stream waits for the caller's stream as it stands
            sees[1][0] = max(sees[1][0], issued[0])
            out.append(None)
        elif l["kind"] == "join":  # the caller's stream waits for the side stream as it stands
            sees[0][1] = max(sees[0][1], issued[1])
            out.append(None)
        else:
            s = l["stream"]
            issued[s] += 1
            sees[s][s] = issued[s]
            out.append((s, issued[s], tuple(sees[s])))
    return out


def before(ca, cb):
    """Whether the launch with clock ca happens before the one with clock cb."""
    s, i, _ = ca
    if ca[0] == cb[0]:
        return i < cb[1]
    return i <= cb[2][s]


# ---- A. layout ----------------------------------------------------------------------------------------------
def check_layout(plan):
    out = []
    subs = sorted({b["sub_batch"] for b in plan["buffers"]})
    for sub in subs:
        rows = [b for b in plan["buffers"] if b["sub_batch"] == sub]
        totals = {b["total"] for b in rows}
        if len(totals) != 1:
            out.append(Violation("A", "total", f"sub {sub}: the rows disagree on the total {sorted(totals)}"))
        total = max(totals)
        for b in rows:
            if b["offset"] % ALIGN:
                out.append(Violation("A", "alignment", f"sub {sub}: {b['name']} at {b['offset']}"))
            if b["offset"] < 0 or b["offset"] + b["bytes"] > total:
                out.append(Violation("A", "buffer-outside-arena", f"sub {sub}: {b['name']} ends at "
                                     f"{b['offset'] + b['bytes']} of {total}"))
        ordered = sorted(rows, key=lambda b: b["offset"])
        for p, q in zip(ordered, ordered[1:]):
            if p["offset"] + p["bytes"] > q["offset"]:
                out.append(Violation("A", "buffers-overlap", f"sub {sub}: {p['name']} ends at {p['offset'] + p['bytes']}, "
                                     f"{q['name']} starts at {q['offset']}"))
        by_id = {b["id"]: b for b in rows}
        for i, l in enumerate(plan["launches"]):
            if l["sub_batch"] != sub:
                continue
            for r in l["ranges"]:
                if r["buffer"] < 0:
                    if r["offset"] < 0 or r["bytes"] <= 0:
                        out.append(Violation("A", "range-empty", f"{name_of(i, l)}: {r}"))
                    continue
                b = by_id.get(r["buffer"])
                if b is None:
                    out.append(Violation("A", "range-unknown-buffer", f"{name_of(i, l)}: {r}"))
                elif r["bytes"] <= 0 or r["offset"] < b["offset"] or r["offset"] + r["bytes"] > b["offset"] + b["bytes"]:
                    out.append(Violation("A", "range-outside-buffer", f"{name_of(i, l)}: {r['role']} [{r['offset']}, "
                                         f"{r['offset'] + r['bytes']}) is not inside {b['name']} [{b['offset']}, "
                                         f"{b['offset'] + b['bytes']})"))
    first = [b["total"] for b in plan["buffers"] if b["sub_batch"] == subs[0]] if subs else []
    for sub in subs[1:]:  # the arena is allocated for the first sub-batch's layout
        t = max(b["total"] for b in plan["buffers"] if b["sub_batch"] == sub)
        if t > max(first):
            out.append(Violation("A", "sub-batch-outgrows-arena", f"sub {sub}: {t} > {max(first)}"))
    return out


# ---- C. hazards ---------------------------------------------------------------------------------------------
def check_hazards(plan):
    out = []
    ls = plan["launches"]
    ck = clocks(ls)
    real = [i for i, c in enumerate(ck) if c is not None]
    for i in real:
        rs = ls[i]["ranges"]
        for a in range(len(rs)):
            for b in range(a + 1, len(rs)):
                if (rs[a]["write"] or rs[b]["write"]) and overlap(rs[a], rs[b]):
                    out.append(Violation("C", "launch-aliases-itself", f"{name_of(i, ls[i])}: {rs[a]['role']} and "
                                         f"{rs[b]['role']} overlap"))
    for x, i in enumerate(real):
        for j in real[x + 1:]:
            if ck[i][0] == ck[j][0] or before(ck[i], ck[j]) or before(ck[j], ck[i]):
                continue
            for r in ls[i]["ranges"]:
                for q in ls[j]["ranges"]:
                    if (r["write"] or q["write"]) and overlap(r, q):
                        out.append(Violation("C", "race", f"{name_of(i, ls[i])} {r['role']} "
                                             f"{'write' if r['write'] else 'read'} and {name_of(j, ls[j])} {q['role']} "
                                             f"{'write' if q['write'] else 'read'} overlap at [{max(r['offset'], q['offset'])}, "
                                             f"{min(span(r)[1], span(q)[1])}) and are not ordered"))
    return out


# ---- D. definition before use ---------------------------------------------------------------------------------
def check_defined(plan):
    out = []
    ls = plan["launches"]
    ck = clocks(ls)
    real = [i for i, c in enumerate(ck) if c is not None]
    for j in real:
        reads = [r for r in ls[j]["ranges"] if not r["write"] and r["buffer"] >= 0]
        if not reads:
            continue
        cover = merged(span(r) for i in real if i != j and ls[i]["sub_batch"] == ls[j]["sub_batch"] and before(ck[i], ck[j])
                       for r in ls[i]["ranges"] if r["write"] and r["buffer"] >= 0)
        for r in reads:
            gaps = uncovered(*span(r), cover)
            if gaps:
                out.append(Violation("D", "read-of-unwritten", f"{name_of(j, ls[j])}: {r['role']} reads "
                                     f"{gaps[:3]} that no earlier launch of its sub-batch wrote"))
    return out


# ---- E. the batch does not choose the arithmetic -----------------------------------------------------------------
def check_splits(plan):
    return [Violation("E", "split-refused", f"{name_of(i, l)}: asked {l['split_asked']}, granted {l['split_granted']}")
            for i, l in enumerate(plan["launches"])
            if l["kind"] not in MARKERS and l["split_granted"] != l["split_asked"]]


def signature(plan, sub):
    """What decides a clip's arithmetic in sub-batch `sub`: per launch, in issue order, (kind, conv, kernel,
    asked split, x_c8, y_c8, relu, residual, stream), the markers included."""
    return [(l["kind"], l["conv"], l["kernel"], l["split_asked"], l["x_c8"], l["y_c8"], l["relu"], l["has_res"], l["stream"])
            for l in plan["launches"] if l["sub_batch"] == sub]


def check_same_arithmetic(plan, one_clip_plan):
    """Every sub-batch of `plan` issues the sequence the one-clip plan does."""
    want = signature(one_clip_plan, 0)
    out = []
    for sub in sorted({l["sub_batch"] for l in plan["launches"]}):
        got = signature(plan, sub)
        if got != want:
            k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            out.append(Violation("E", "sequence-depends-on-batch", f"sub {sub}: launch {k}: "
                                 f"{got[k] if k < len(got) else None} != one clip's {want[k] if k < len(want) else None}"))
    return out


# ---- F. sub-batch sizes ---------------------------------------------------------------------------------------
def sub_batch_clips(plan):
    clips = {}
    for b in plan["buffers"]:
        clips.setdefault(b["sub_batch"], set()).add(b["clips"])
    return [sorted(clips[s]) for s in sorted(clips)]


def check_sub_batches(plan, n, max_clips):
    want = [[max_clips]] * (n // max_clips) + ([[n % max_clips]] if n % max_clips else [])
    got = sub_batch_clips(plan)
    return [] if got == want else [Violation("F", "sub-batch-sizes", f"{got} != {want}")]


def audit(plan):
    """Checks A, C, D and the split half of E: everything a plan can be asked on its own."""
    return check_layout(plan) + check_hazards(plan) + check_defined(plan) + check_splits(plan)


# ---- B. footprints from independent arithmetic --------------------------------------------------------------------
def elem(dtype):
    return 2 if "bfloat16" in str(dtype) else 4


def expected_convs(table, n, t, h, w, out_dim):
    """{conv index: {"x", "x2", "res", "y": bytes, "m": output voxels, "cout_p"}} for a forward of n clips of
    (t, h, w), from the conv table's padded channels, kernel, stride and padding and out_dim alone. The
    topology is the reference network's: two stem convs, then blocks of four convs (the fourth adds the
    block's input, or a 1x1x1 downsample conv of it where one follows in the table), two blocks per layer;
    the last four rows are the projections of (stem tap, layer1 tap), layer2, layer3 and layer4 taps."""
    backbone, proj = table[:-4], table[-4:]

    def through(c, s):
        return tuple(out_dim(d, k, st, p) for d, k, st, p in zip(s, c["kernel"], c["stride"], c["padding"]))

    def vox(s):
        return n * s[0] * s[1] * s[2]

    exp = {}

    def conv(c, s, res=False):
        o = through(c, s)
        xe, ye = elem(c["in_dtype"]), elem(c["out_dtype"])
        exp[c["index"]] = {"x": vox(s) * c["cin_p"] * xe, "x2": vox(s) * c["cin2"] * xe,
                           "res": vox(o) * c["cout_p"] * ye if res else 0, "y": vox(o) * c["cout_p"] * ye,
                           "m": vox(o), "cout_p": c["cout_p"], "xe": xe, "ye": ye}
        return o

    s = conv(backbone[1], conv(backbone[0], (t, h, w)))
    taps = [s]
    i, blocks = 2, 0
    while i < len(backbone):
        block_in = s
        for k in range(3):
            s = conv(backbone[i + k], s)
        s = conv(backbone[i + 3], s, res=True)
        i += 4
        if i < len(backbone) and backbone[i]["kernel"] == (1, 1, 1):
            assert conv(backbone[i], block_in) == s
            i += 1
        blocks += 1
        if blocks % 2 == 0:
            taps.append(s)
    assert len(taps) == 5
    for c, tap in zip(proj, (taps[0], taps[2], taps[3], taps[4])):
        conv(c, tap)
    return exp


def check_footprints(plan, table, n_of_sub, t, h, w, out_dim, tap_shapes):
    """B: the plan's ranges against expected_convs, the pack's and the decoder's exact sizes. n_of_sub: clips
    of each sub-batch."""
    out = []
    for sub, n in enumerate(n_of_sub):
        exp = expected_convs(table, n, t, h, w, out_dim)
        seen = {}
        for i, l in enumerate(l for l in plan["launches"] if l["sub_batch"] == sub):
            got = {}
            for r in l["ranges"]:
                got[(r["role"], r["write"])] = got.get((r["role"], r["write"]), [])
                got[(r["role"], r["write"])].append(r["bytes"])
            bad = lambda what: out.append(Violation("B", "footprint", f"sub {sub} {name_of(i, l)}: {what}; ranges {l['ranges']}"))
            if l["kind"] == "pack":
                if got != {("x", False): [n * 3 * t * h * w * 4], ("y", True): [n * t * h * w * 4 * 4]}:
                    bad("pack reads the clips and writes N*T*H*W*4 floats")
            elif l["kind"] == "dec_index":
                if set(got) != {("idx", True)}:
                    bad("the index kernel writes the table only")
            elif l["kind"] == "decoder":
                want = {("tap", False): [n * a * b * c * 64 * 4 for a, b, c in tap_shapes(t, h, w)],
                        ("y", True): [n * 2 * t * h * w * 4, n * 4 * t * h * w * 4]}
                idx = got.pop(("idx", False), None)
                if got != want or idx is None or len(idx) != 1:
                    bad(f"the decoder reads four fp32 taps {want[('tap', False)]} and the table, and writes seg and motion")
            elif l["kind"] in ("conv", "split_sum"):
                e = exp.get(l["conv"])
                if e is None:
                    bad("unknown conv")
                    continue
                part = l["split_granted"] * e["m"] * e["cout_p"] * 4
                if (l["x_elem"], l["y_elem"]) != (e["xe"], e["ye"]):
                    bad(f"element sizes {(l['x_elem'], l['y_elem'])} != {(e['xe'], e['ye'])}")
                if bool(l["has_res"]) != bool(e["res"]):
                    bad("residual")
                epilogue = {("y", True): [e["y"]], **({("res", False): [e["res"]]} if e["res"] else {})}
                inputs = {("x", False): [e["x"]], **({("x2", False): [e["x2"]]} if e["x2"] else {})}
                if l["kind"] == "conv":
                    want = {**inputs, **(epilogue if l["split_granted"] == 1 else {("part", True): [part]})}
                    seen[l["conv"]] = seen.get(l["conv"], 0) + 1
                else:
                    want = {("part", False): [part], **epilogue}
                    if l["split_granted"] < 2:
                        bad("a split sum without a split")
                if got != want:
                    bad(f"expected {want}")
            elif l["kind"] not in MARKERS:
                bad("unknown kind")
        if seen != {k: 1 for k in exp}:
            out.append(Violation("B", "convs-launched", f"sub {sub}: every conv once, got {seen}"))
    return out


def check_split_sums(plan):
    """A split sum follows exactly each conv launch that was granted a split, on its stream, for its conv."""
    out = []
    ls = [l for l in plan["launches"] if l["kind"] not in MARKERS]
    for i, l in enumerate(ls):
        nxt = ls[i + 1] if i + 1 < len(ls) else None
        follows = nxt is not None and nxt["kind"] == "split_sum" and (nxt["conv"], nxt["stream"], nxt["sub_batch"]) == (
            l["conv"], l["stream"], l["sub_batch"])
        if l["kind"] == "conv" and (l["split_granted"] > 1) != follows:
            out.append(Violation("B", "split-sum-placement", name_of(i, l)))
        if l["kind"] == "split_sum" and (i == 0 or ls[i - 1]["kind"] != "conv"):
            out.append(Violation("B", "split-sum-placement", name_of(i, l)))
    return out


# ---- what a forward leaves in the arena (tests/test_plan_gpu.py) ---------------------------------------------------
def written_elements(plan):
    """Disjoint, sorted (a, b, element bytes or None) over the union of the plan's arena writes: the element
    size is the last writer's in issue order (None for the decoder's index table, whose entries are not
    activations). Issue order is the final state's order because check C allows no unordered overlap."""
    pieces = []  # disjoint, unsorted
    for l in plan["launches"]:
        for r in l["ranges"]:
            if not r["write"] or r["buffer"] < 0:
                continue
            a, b = span(r)
            size = {"y": l["y_elem"], "part": 4}.get(r["role"])
            kept = []
            for pa, pb, ps in pieces:
                if pb <= a or pa >= b:
                    kept.append((pa, pb, ps))
                    continue
                if pa < a:
                    kept.append((pa, a, ps))
                if pb > b:
                    kept.append((b, pb, ps))
            kept.append((a, b, size))
            pieces = kept
    return sorted(pieces)
