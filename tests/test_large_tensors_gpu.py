"""Tensors past 2 GiB: every conv kernel with a 32-bit addressing limit is run one clip short of that limit
and asked for one clip past it, and the whole forward is run one clip past the largest batch a single pass
of the network takes (Engine.max_clips, DESIGN.md "Size limits").

Oracle: a conv is local to a clip and its kernel and geometry are chosen from the per-clip shape, so clip i
run alone is an exact oracle for clip i of a batch. Every per-clip shape here is one test_layers_gpu.CASES
already holds to float64; this file compares bits (int32 / int16 views), never tolerances.

Fill: signed values of magnitude in [0.5, 1], drawn on the device (LR.signed_unit's distribution), so a
padding pixel that read real data, or a clip that read its neighbour, changes an output.

Contract chosen for the F(4x4,3x3) kernels (conv_wino4r, conv_wino4w, conv_wino4), whose padding slot is
byte offset 2^31 of the input: an input of 2^31 bytes or more is refused (CLASFV_EBADSHAPE, nothing
launched), never handed to a kernel of another rounding family. The bit-identical switches a launcher makes
inside one kernel stay and are crossed: conv_winot5 -> conv_winot at 2^32 input bytes (channels-last input),
buffer -> pointer DMAs of conv_dma_x3 / conv_dma at 2^31. conv_dma_w -> conv_dma at 2^31 would change the
kernel's name with the batch and is refused; so is a blocked mid tensor of 2^32 bytes in the forward.

A refused call is given buffers of the full size all the same: were the refusal missing, the launch would
still stay inside the allocations (a wrong result, not a stray access).

Memory: a case allocates at most 24 GiB and frees it before the next; it skips only when the device reports
less free memory than it needs, and prints both figures. Wall times and peaks: profiles/
large_tensor_tests_mi355x.txt.
"""
import ctypes
import gc
import time

import pytest
import torch

from clasfv_amd import _lib
from tests import test_layers_gpu as TL

pytestmark = pytest.mark.gpu

GUARD = TL.GUARD
CAP = 24 << 30  # bytes a case may allocate
LIM31, LIM32 = 1 << 31, 1 << 32


def need(nbytes, what):
    """Skip (only) when the device has less free memory than the case needs; never ask for more than CAP."""
    assert nbytes <= CAP, f"{what}: needs {nbytes} B, above the {CAP} B a case may allocate"
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        print(f"{what}: needs {nbytes} B of device memory, {free} B free")
        pytest.skip(f"{what}: needs {nbytes} B of device memory, {free} B free")


def fill_signed_unit(t, seed):
    """t (fp32 or bf16, on the device) <- random signs x magnitudes uniform in [0.5, 1], in place, chunked."""
    gen = torch.Generator(device=t.device).manual_seed(seed)
    flat = t.view(-1)
    step = 1 << 26
    for a in range(0, flat.numel(), step):
        part = flat[a:a + step]
        mag = torch.empty(part.numel(), dtype=torch.float32, device=t.device).uniform_(0.5, 1.0, generator=gen)
        sign = torch.empty(part.numel(), dtype=torch.int8, device=t.device).random_(0, 2, generator=gen)
        part.copy_(mag * (sign.float() * 2 - 1))
    bits = flat.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    return bits


def bits_of(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def all_set(bits):
    """Every element still holds the all-ones sentinel (chunked: no full-size temporary)."""
    step = 1 << 28
    return all(bool((bits[a:a + step] == -1).all()) for a in range(0, bits.numel(), step))


def none_set(bits):
    step = 1 << 28
    return all(bool((bits[a:a + step] != -1).all()) for a in range(0, bits.numel(), step))


def out_shape(e, thw):
    from oracle import layer_ref as LR
    return tuple(LR.out_dim(d, k, s, p) for d, k, s, p in zip(thw, e["kernel"], e["stride"], e["padding"]))


def clip_view(y, n, vox, c, c8):
    """Output tensor of n clips as [n][...]: channels-last (n, vox, c) or blocked (c/8, n, vox, 8) -> clip i."""
    if c8:
        return lambda i: y.view(c // 8, n, vox, 8)[:, i]
    return lambda i: y.view(n, vox, c)[i]


class Big:
    """One conv of the table over n clips of thw between guard bands: inputs filled, output all ones."""

    def __init__(self, nt, layer, thw, n, x_c8=False, y_c8=False, seed=1):
        self.nt, self.e = nt, nt.by_name[layer]
        e = self.e
        self.thw, self.n, self.x_c8, self.y_c8 = thw, n, x_c8, y_c8
        self.vin = thw[0] * thw[1] * thw[2]
        self.oshape = out_shape(e, thw)
        self.vout = self.oshape[0] * self.oshape[1] * self.oshape[2]
        dev = nt.engine.device
        es_in, es_out = (2 if e["in_dtype"] == torch.bfloat16 else 4), (2 if e["out_dtype"] == torch.bfloat16 else 4)
        nin, nout = n * self.vin * e["cin_p"], n * self.vout * e["cout_p"]
        # inputs, output, and the temporaries of filling (2^26-element chunks) and checking (2^28 flags)
        need(nin * es_in + nout * es_out + (2 << 30), f"{layer} x {n} clips")
        self.xbuf, self.xbits_all, self.x = TL.guarded(nin, e["in_dtype"], dev)
        fill_signed_unit(self.x, seed)
        if e["cin_p"] != e["cin"]:  # padded input channels are zero, as the engine's producers leave them
            assert not x_c8
            self.x.view(-1, e["cin_p"])[:, e["cin"]:] = 0
        self.ybuf, self.ybits_all, self.y = TL.guarded(nout, e["out_dtype"], dev)
        self.nout = nout

    def run(self, flags=(), relu=False, n=None, x=None, y=None, x_c8=None):
        """clasfv_run_conv over the whole batch (or over n clips at x into y); (rc, kernel name, launch log)."""
        eng, e = self.nt.engine, self.e
        x_c8 = self.x_c8 if x_c8 is None else x_c8
        n = self.n if n is None else n
        x = self.x if x is None else x
        y = self.y if y is None else y
        name = ctypes.c_char_p()
        old = eng.set_variants(*flags)
        eng.set_launch_log(True)
        try:
            def go():
                rc = eng.lib.clasfv_run_conv(eng.h, e["index"], _lib.ptr(x), n, *self.thw, None, None, int(relu),
                                             int(x_c8), int(self.y_c8), _lib.ptr(y), None, 0, ctypes.byref(name),
                                             _lib.stream_ptr(None, eng.device))
                if rc not in (0, -2):
                    _lib.check(rc, "clasfv_run_conv")
                torch.cuda.synchronize()
                return rc
            rc = TL.on_device(go)
            log = eng.launch_log()
        finally:
            eng.set_launch_log(False)
            eng.set_variants(*old)
        return rc, (name.value or b"").decode(), log

    def single(self, i, flags=(), relu=False):
        """Clip i alone (its own input, channels-last, and a fresh guarded output): the oracle."""
        e = self.e
        if self.x_c8:  # clip i's voxels of every 8-channel block, gathered
            xi = self.x.view(e["cin_p"] // 8, self.n, self.vin, 8)[:, i].permute(1, 0, 2).reshape(-1).contiguous()
        else:
            xi = self.x.view(self.n, self.vin * e["cin_p"])[i]
        _, ybits, y1 = TL.guarded(self.vout * e["cout_p"], e["out_dtype"], xi.device)
        rc, name, log = self.run(flags, relu, n=1, x=xi, y=y1, x_c8=False)
        assert rc == 0 and TL.guards_intact(ybits)
        return y1, name, log

    def check_written(self):
        e = self.e
        assert TL.guards_intact(self.xbits_all), "an input guard band was written"
        assert TL.guards_intact(self.ybits_all), "write outside the output tensor"
        assert none_set(bits_of(self.y)), "output elements left unwritten"
        if e["cout_p"] != e["cout"]:
            if self.y_c8:  # the tail of the first block that holds a padded channel, and every block after it
                rows = self.y.view(e["cout_p"] // 8, -1, 8)
                first = e["cout"] // 8
                pad_bits = torch.cat([bits_of(rows[first][:, e["cout"] % 8:].contiguous()).reshape(-1)] +
                                     [bits_of(rows[b]).reshape(-1) for b in range(first + 1, e["cout_p"] // 8)])
            else:
                pad_bits = bits_of(self.y.view(-1, e["cout_p"])[:, e["cout"]:].contiguous())
            assert bool((pad_bits == 0).all()), "padded output channels are not exactly +0"

    def check_refused(self, rc, log):
        assert rc == -2, f"expected CLASFV_EBADSHAPE, got {rc}"
        assert log == [], f"a refused call launched {log}"
        assert all_set(bits_of(self.y)) and TL.guards_intact(self.ybits_all), "a refused call wrote its output"

    def check_clips(self, clips, flags=(), relu=False):
        """Clips of the batch's output equal their single-clip runs bit for bit; returns the oracles' names."""
        e = self.e
        view = clip_view(self.y, self.n, self.vout, e["cout_p"], self.y_c8)
        names = set()
        for i in clips:
            y1, name, _ = self.single(i, flags, relu)
            names.add(name)
            want = (y1.view(e["cout_p"] // 8, 1, self.vout, 8)[:, 0] if self.y_c8 else y1.view(self.vout, e["cout_p"]))
            got = view(i)
            same = torch.equal(bits_of(got.contiguous()), bits_of(want.contiguous()))
            assert same, f"clip {i} of {self.n} differs from its single-clip run " \
                         f"({int((bits_of(got.contiguous()) != bits_of(want.contiguous())).sum())} of {want.numel()} elements)"
        return names


def clips_around(limit_bytes, clip_bytes):
    """(the largest N whose input ends below the limit, N + 2: the clip holding the limit byte and one more)."""
    below = (limit_bytes - 1) // clip_bytes
    return below, below + 2


# ---- a. isolated convs across each byte threshold ---------------------------------------------------------
F44 = [  # (layer, per-clip shape, kernel, flags, y_c8): each a per-clip shape of test_layers_gpu.CASES
    ("layer1.0.conv1.0.0", (4, 12, 12), "conv_wino4r", (), False),
    ("layer1.0.conv1.0.0", (4, 12, 12), "conv_wino4r", (), True),
    ("layer1.0.conv1.0.0", (4, 10, 14), "conv_wino4w", ("no_wino4r",), False),
    ("layer1.0.conv1.0.0", (4, 10, 14), "conv_wino4", ("no_wino4w",), False),
    ("layer2.0.conv2.0.0", (4, 12, 12), "conv_wino4", (), False),
    ("layer2.0.conv2.0.0", (4, 12, 12), "conv_wino4", (), True),
]


def f44_id(c):
    return f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}" + ("-yc8" if c[4] else "")


@pytest.mark.parametrize("past", (False, True), ids=("below", "past"))
@pytest.mark.parametrize("c", F44, ids=f44_id)
def test_f44_conv_at_the_padding_slot(c, past):
    """The F(4x4,3x3) kernels' "read zeros" slot is byte 2^31 of the input. One clip short of it the batch runs
    and its first, last and a middle clip equal their single-clip runs; with the slot inside the input (the
    clip holding byte 2^31, and one more) the call is refused and nothing is launched or written."""
    layer, thw, kernel, flags, y_c8 = c
    nt = TL.net("fp32", "float")
    e = nt.by_name[layer]
    clip = thw[0] * thw[1] * thw[2] * e["cin_p"] * 4
    below, above = clips_around(LIM31, clip)
    assert below * clip < LIM31 <= (below + 1) * clip
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    b = Big(nt, layer, thw, above if past else below, y_c8=y_c8, seed=7)
    rc, name, log = b.run(flags)
    assert name == kernel, f"kernel of one clip of the shape: {name}"
    if past:
        b.check_refused(rc, log)
    else:
        assert rc == 0
        assert {TL.label_kernel(lb) for lb, _, _, _ in log} == {kernel}
        b.check_written()
        assert b.check_clips((0, below // 2, below - 1), flags) == {kernel}
    print(f"LARGE {f44_id(c)} {'past' if past else 'below'} N={b.n} in={b.n * clip} B "
          f"peak={torch.cuda.max_memory_allocated()} B wall={time.time() - t0:.2f} s")


@pytest.mark.parametrize("past", (False, True), ids=("below", "past"))
def test_winot5_hands_over_to_winot_at_4_gib(past):
    """conv_winot5 offsets its input in 32-bit bytes: below 2^32 input bytes launch_winot takes it (here over the
    8-channel-blocked layout, as in the forward), from there conv_winot, channels-last only. Both report
    conv_winot; the launch log tells them apart. Past the threshold the bits equal the winot_reference
    form's, and each checked clip equals its single-clip run, which conv_winot5 computes."""
    layer, thw = "layer1.0.conv1.0.3", (8, 9, 9)
    nt = TL.net("fp32", "float")
    e = nt.by_name[layer]
    clip = thw[0] * thw[1] * thw[2] * e["cin_p"] * 4
    below, above = clips_around(LIM32, clip)
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    if not past:
        b = Big(nt, layer, thw, below, x_c8=True, seed=8)
        rc, name, log = b.run()
        assert rc == 0 and name == "conv_winot"
        assert {TL.label_kernel(lb) for lb, _, _, _ in log} == {"conv_winot5"}
        b.check_written()
        for i in (0, below // 2, below - 1):
            y1, _, log1 = b.single(i)
            assert {TL.label_kernel(lb) for lb, _, _, _ in log1} == {"conv_winot5"}
            assert torch.equal(bits_of(b.y.view(below, -1)[i]), bits_of(y1)), f"clip {i} differs from its single-clip run"
    else:
        b = Big(nt, layer, thw, above, seed=8)
        rc, name, log = b.run()
        assert rc == 0 and name == "conv_winot"
        assert {TL.label_kernel(lb) for lb, _, _, _ in log} == {"conv_winot"}
        b.check_written()
        holder = LIM32 // clip  # the clip holding byte 2^32
        for i in (0, holder, above - 1):
            y1, _, log1 = b.single(i)
            assert {TL.label_kernel(lb) for lb, _, _, _ in log1} == {"conv_winot5"}
            assert torch.equal(bits_of(b.y.view(above, -1)[i]), bits_of(y1)), f"clip {i} differs from its single-clip run"
        # the blocked layout is conv_winot5's alone: past its limit it is refused, and nothing is launched
        snap = bits_of(b.y)[:1 << 20].clone()
        rcx, _, logx = b.run(x_c8=True)
        assert rcx == -2 and logx == [] and torch.equal(bits_of(b.y)[:1 << 20], snap)
        # the reference form, on the same batch
        keep = bits_of(b.y)[:b.vout * e["cout_p"] * 64].clone()
        last = bits_of(b.y)[-b.vout * e["cout_p"] * 64:].clone()
        bits_of(b.y).fill_(-1)
        rc, name, log = b.run(("winot_reference",))
        assert rc == 0 and {TL.label_kernel(lb) for lb, _, _, _ in log} == {"conv_winot"}
        assert torch.equal(bits_of(b.y)[:keep.numel()], keep) and torch.equal(bits_of(b.y)[-last.numel():], last)
    print(f"LARGE winot-{'past' if past else 'below'} N={b.n} in={b.n * clip} B "
          f"peak={torch.cuda.max_memory_allocated()} B wall={time.time() - t0:.2f} s")


DMA = [  # (dtype, layer, per-clip shape, flags, kernel below, kernel past; None: the batch is refused)
    ("fp32", "layer2.0.downsample.0", (5, 13, 11), (), "conv_dma_x3", "conv_dma_x3"),
    ("bf16", "P3", (3, 10, 14), (), "conv_dma_w", None),
    ("bf16", "P3", (3, 10, 14), ("no_dma_w",), "conv_dma", "conv_dma"),
]


@pytest.mark.parametrize("past", (False, True), ids=("below", "past"))
@pytest.mark.parametrize("c", DMA, ids=lambda c: f"{c[0]}-{c[1]}-{c[4]}")
def test_dma_buffer_form_ends_at_2_gib(c, past):
    """The buffer-offset DMAs of conv_dma_x3, conv_dma_w and conv_dma address 2^31 bytes: past that the launch
    log shows the pointer instantiation (the one no_dma_buf launches for a single clip), the bits equal the
    no_dma_buf run's, and the checked clips equal their single-clip runs, which the buffer form computes.
    conv_dma_w has no pointer form: conv_dma would take its batch, bit for bit the same, but a batch does not
    change the kernel a clip runs on (the launch plan's check E), so it is refused, and no_dma_w serves it."""
    dtype, layer, thw, flags, k_below, k_past = c
    nt = TL.net(dtype, "float")
    e = nt.by_name[layer]
    es = 2 if e["in_dtype"] == torch.bfloat16 else 4
    clip = thw[0] * thw[1] * thw[2] * e["cin_p"] * es
    below, above = clips_around(LIM31, clip)
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    b = Big(nt, layer, thw, above if past else below, seed=9)
    rc, name, log = b.run(flags, relu=False)
    if past and k_past is None:
        assert name == k_below
        b.check_refused(rc, log)
        print(f"LARGE dma-{dtype}-{layer}-{k_below}-past N={b.n} in={b.n * clip} B refused wall={time.time() - t0:.2f} s")
        return
    assert rc == 0 and name == (k_past if past else k_below)
    labels = {lb for lb, _, _, _ in log}
    assert len(labels) == 1
    _, _, log_buf = b.single(0, flags, relu=False)
    _, _, log_ptr = b.single(0, flags + ("no_dma_buf",), relu=False)
    buf_form, ptr_form = {lb for lb, _, _, _ in log_buf}, {lb for lb, _, _, _ in log_ptr}
    assert buf_form != ptr_form and len(ptr_form) == 1
    assert labels == (ptr_form if past else buf_form), f"launched {labels}"
    b.check_written()
    clips = (0, LIM31 // clip, above - 1) if past else (0, below // 2, below - 1)
    b.check_clips(clips, flags, relu=False)
    if past:
        n_keep = b.vout * e["cout_p"] * 64
        keep, last = bits_of(b.y)[:n_keep].clone(), bits_of(b.y)[-n_keep:].clone()
        bits_of(b.y).fill_(-1)
        rc, _, log2 = b.run(flags + ("no_dma_buf",), relu=False)
        assert rc == 0 and {lb for lb, _, _, _ in log2} == ptr_form
        assert torch.equal(bits_of(b.y)[:n_keep], keep) and torch.equal(bits_of(b.y)[-n_keep:], last)
    print(f"LARGE dma-{dtype}-{layer}-{k_below}-{'past' if past else 'below'} N={b.n} in={b.n * clip} B "
          f"peak={torch.cuda.max_memory_allocated()} B wall={time.time() - t0:.2f} s")


# ---- b. the whole forward across the sub-batch limit ------------------------------------------------------
# max_clips by the table of DESIGN.md "Size limits": fp32, layer1's 144-channel mid tensor, 8-channel-blocked for
# conv_winot5, stays below 2^32 bytes: N * T * (H/2) * (W/2) * 144 * 4 < 2^32. The blocked layout is one clip's
# choice (the launch plan's check E): a batch does not switch it off, it is refused. With channels-last mid
# tensors (no_c8) the 64-channel input of layer1's F(4x4) convs below 2^31 bytes binds, N * T * (H/2) * (W/2) *
# 64 * 4 < 2^31, and below that limit the mid tensor passes 2^32 bytes inside one pass.
FORWARD = [("fp32", (64, 224, 224), 9, ()), ("fp32", (32, 112, 112), 74, ()), ("fp32", (32, 112, 112), 83, ("no_c8",))]


@pytest.mark.parametrize("dtype,thw,want,variants", FORWARD,
                         ids=[f"{d}-{'x'.join(map(str, s_))}{''.join('-' + v for v in vs)}" for d, s_, _, vs in FORWARD])
def test_forward_one_clip_past_the_sub_batch_limit(dtype, thw, want, variants):
    """N = max_clips + 1 runs as two passes over the conv table (max_clips clips, then one) in the workspace of
    max_clips clips, and clips 0, max_clips - 1 and max_clips equal their single-clip forwards bit for bit.
    Every pass runs conv_winot5 over the blocked layout, as a single clip does. With no_c8, max_clips - 1 clips
    are also past 2^32 bytes of layer1's channels-last mid tensor, so the first pass runs conv_winot where the
    single clips run conv_winot5."""
    t, h, w = thw
    nt = TL.Net(dtype, "float")  # a handle of its own: the workspace it holds is this test's
    eng = nt.engine
    eng.set_variants(*variants)
    mc = eng.max_clips(t, h, w)
    vox = t * (h // 2) * (w // 2)
    assert mc == want == ((LIM31 - 1) // (vox * 64 * 4) if variants else (LIM32 - 1) // (vox * 144 * 4))
    n = mc + 1
    clip = t * h * w
    # the workspace of mc clips (make_layout: just under 150 floats per input voxel), input, outputs, fill
    need(mc * clip * 600 + n * clip * 9 * 4 + (1 << 30), f"forward {dtype} {thw} x {n}")
    dev = eng.device
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    x = torch.empty((n, 3, t, h, w), dtype=torch.float32, device=dev)
    fill_signed_unit(x, 10)
    seg = torch.empty((n, 2, t, h, w), dtype=torch.float32, device=dev)
    mot = torch.empty((n, 4, t, h, w), dtype=torch.float32, device=dev)

    def fwd(xx, ss, mm):
        def go():
            eng.forward(xx, ss, mm)
            torch.cuda.synchronize()
        TL.on_device(go)

    fwd(x[:mc], seg[:mc], mot[:mc])
    ws = eng.workspace_bytes()
    bits_of(seg).fill_(-1)
    bits_of(mot).fill_(-1)
    eng.set_launch_log(True)
    fwd(x, seg, mot)
    log = eng.launch_log(cap=1 << 12)
    eng.set_launch_log(False)
    assert eng.workspace_bytes() == ws, "the workspace grew past that of max_clips clips"
    packs = [i for i, (lb, _, _, _) in enumerate(log) if TL.label_kernel(lb) == "pack_input_kernel"]
    assert len(packs) == 2 and packs[0] == 0, "two passes over the network"
    first, second = log[:packs[1]], log[packs[1]:]
    convs = lambda part: [cv for _, _, _, cv in part if cv >= 0]
    n_convs = len(eng.conv_table())
    assert sorted(set(convs(first))) == sorted(set(convs(second))) == list(range(n_convs))
    assert none_set(bits_of(seg)) and none_set(bits_of(mot))
    winot = lambda part: {TL.label_kernel(lb) for lb, _, _, cv in part if TL.label_kernel(lb).startswith("conv_winot")}
    if dtype == "fp32":
        assert winot(first) == ({"conv_winot", "conv_winot5"} if variants else {"conv_winot5"})
        assert winot(second) == {"conv_winot5"}
    s1 = torch.empty((1, 2, t, h, w), dtype=torch.float32, device=dev)
    m1 = torch.empty((1, 4, t, h, w), dtype=torch.float32, device=dev)
    for i in (0, mc - 1, mc):
        bits_of(s1).fill_(-1)
        bits_of(m1).fill_(-1)
        fwd(x[i:i + 1], s1, m1)
        assert torch.equal(bits_of(seg[i:i + 1]), bits_of(s1)), f"clip {i}: segmentation logits differ from the single-clip forward"
        assert torch.equal(bits_of(mot[i:i + 1]), bits_of(m1)), f"clip {i}: motion differs from the single-clip forward"
    assert eng.workspace_bytes() == ws
    print(f"LARGE forward-{dtype}-{t}x{h}x{w} max_clips={mc} N={n} workspace={ws} B "
          f"peak={torch.cuda.max_memory_allocated()} B wall={time.time() - t0:.2f} s")


# ---- c. refusals ------------------------------------------------------------------------------------------
def small_forward(eng):
    dev = eng.device
    gen = torch.Generator().manual_seed(3)
    x = torch.rand((2, 3, 8, 32, 32), generator=gen).to(dev)
    seg = torch.empty((2, 2, 8, 32, 32), device=dev)
    mot = torch.empty((2, 4, 8, 32, 32), device=dev)
    eng.forward(x, seg, mot)
    torch.cuda.synchronize()
    return bits_of(seg).clone(), bits_of(mot).clone()


@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_oversize_shapes_are_refused_before_any_launch(dtype):
    """Pure argument checks: none of these entry points reads a tensor before it refuses, so the buffers are
    small and the dimensions large. Each returns CLASFV_EBADSHAPE with an empty launch log and untouched
    outputs, and the handle computes the same small forward after as before."""
    nt = TL.net(dtype, "float")
    eng = nt.engine
    dev = eng.device
    before = small_forward(eng)
    _, ybits, y = TL.guarded(1 << 16, torch.float32, dev)
    x = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    sp = _lib.stream_ptr(None, dev)
    eng.set_launch_log(True)
    try:
        # clasfv_run_conv: 2^31 output voxels (M is an int), on a conv of each kind of last resort
        for layer, nthw in (("layer1.0.conv1.0.0", (1 << 19, 4, 32, 32)), ("layer2.0.downsample.0", (1 << 21, 8, 16, 16)),
                            ("P4", (1 << 21, 4, 16, 16)), ("stem.0", (1 << 15, 8, 256, 256))):
            e = nt.by_name[layer]
            name = ctypes.c_char_p()
            rc = eng.lib.clasfv_run_conv(eng.h, e["index"], _lib.ptr(x), *nthw, None, None, 1, 0, 0, _lib.ptr(y), None, 0,
                                         ctypes.byref(name), sp)
            assert rc == -2, f"{layer} {nthw}: {rc} {eng.lib.clasfv_last_error()}"
            assert eng.launch_log() == []
        # clasfv_run_conv past a kernel's own limit with M far below 2^31: the temporal conv's 2^31 elements
        # (fp32: conv_winot; bf16: conv_twalk_bf16) at 144 / 160 channels
        e = nt.by_name["layer1.0.conv1.0.3"]
        n_el = LIM31 // (8 * 16 * 16 * e["cin_p"]) + 1
        rc = eng.lib.clasfv_run_conv(eng.h, e["index"], _lib.ptr(x), n_el, 8, 16, 16, None, None, 1, 0, 0, _lib.ptr(y), None,
                                     0, None, sp)
        assert rc == -2 and eng.launch_log() == [], eng.lib.clasfv_last_error()
        # clasfv_run_decoder: a P01 tap of 2^31 floats (42 clips of 64 x 224 x 224), and one float fewer is
        # not refused for its size (41 clips: the same check passes; not run, the buffers are small)
        per_clip = 64 * 112 * 112 * 64
        n_tap = -(-LIM31 // per_clip)
        assert (n_tap - 1) * per_clip < LIM31 <= n_tap * per_clip and n_tap == 42
        rc = eng.lib.clasfv_run_decoder(eng.h, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), n_tap, 64, 224, 224,
                                        _lib.ptr(y), _lib.ptr(y), sp)
        assert rc == -2 and eng.launch_log() == [], eng.lib.clasfv_last_error()
        ws = eng.workspace_bytes()
        # clasfv_forward: one clip of 2^31 voxels (M >= 2^31 at the very first conv): no sub-batch serves it
        rc = eng.lib.clasfv_forward(eng.h, _lib.ptr(x), 1, 8, 16384, 16384, _lib.ptr(y), _lib.ptr(y), sp)
        assert rc == -2 and eng.launch_log() == [], eng.lib.clasfv_last_error()
        assert eng.workspace_bytes() == ws, "a refused forward allocated a workspace"
        assert eng.max_clips(8, 16384, 16384) == 0
    finally:
        eng.set_launch_log(False)
    torch.cuda.synchronize()
    assert all_set(ybits), "a refused call wrote its output"
    after = small_forward(eng)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
