"""The blocked-stream protocol of tests/test_stream_order_gpu.py ("Stream order").

A call under test is issued on a non-blocking stream S whose head is held by a finite sleep kernel (the
blocker). Behind the blocker, still on S, device-to-device copies replace the "stale" inputs A' that the
buffers hold with the real inputs A; then the call is made. Two things follow:

* the blocker has not finished when the call returns, or the call waited for the device (or took longer than
  a blocker of 50 times its measured host time, which is reported as the same failure);
* after S is synchronised the outputs equal R(A), the serial result on the default stream, bit for bit. Any
  launch, memset or copy of the call that went to another stream than S ran while the buffers held A' and the
  scratch held what the last call left there, so the output then differs from R(A): the test first asserts
  that R(A) != R(A').

A' is always valid input of the same shapes (labels in range, finite floats, tables inside the video), so a
defect shows as a wrong answer, never as a fault. The blocker ends by itself: nothing here waits for a flag.
"""
import ctypes
import time

import pytest
import torch

SENTINEL_U8 = 0xA5                   # labels are 0, 1 or 2; wider elements get all-ones bits (a NaN as a float)
MIN_BLOCK, MAX_BLOCK = 0.25, 1.0     # seconds
HOST_FACTOR = 50                     # blocker length in units of the call's measured host time
EHIP = -4
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_state = {}


def dev():
    return torch.device("cuda", 0)


def _runs_beside(first, other):
    """Does a trivial kernel on ``other`` complete while a short blocker holds ``first``?"""
    flag = torch.zeros(1, device=dev())
    sync()
    blocker = Blocker(first, 0.03)
    with torch.cuda.stream(other):
        flag.add_(1)
    sync(other)
    beside = blocker.running()
    sync(first)
    return beside


def side_streams():
    """The two non-default streams every case of the session uses (with the default stream: three contexts
    per engine handle, under the four it keeps). Made once: each torch.cuda.Stream() is another HIP stream.
    Some pairs of streams run in turn whatever the library does (measured; supposedly because the runtime
    serves its streams from a few hardware queues). So the first stream is the first of up to eight candidates beside which the
    default stream runs a trivial kernel while a short blocker holds the candidate (the references, the
    comparisons and the clip-table test work on the default stream while the first stream is blocked), and
    the second is the first of up to eight that run beside the first (the two-stream cases need such a pair,
    and fail, naming this, if there is none)."""
    if "streams" not in _state:
        null = torch.cuda.default_stream(dev())
        for i in range(8):
            s1 = torch.cuda.Stream(dev())
            beside_null = _runs_beside(s1, null)
            if beside_null:
                break
        for j in range(8):
            s2 = torch.cuda.Stream(dev())
            found = _runs_beside(s1, s2)
            if found:
                break
        print(f"STREAM_PAIR first stream: candidate {i}, the default stream runs beside it: {beside_null}; "
              f"second stream: candidate {j}, runs beside the first: {found}")
        _state["streams"], _state["concurrent"], _state["null_concurrent"] = (s1, s2), found, beside_null
    return _state["streams"]


def streams_are_concurrent():
    side_streams()
    return _state["concurrent"]


def default_stream_is_concurrent():
    side_streams()
    return _state["null_concurrent"]


def current_ptr():
    """hipStream_t of the current stream, taken here and not through the package's own helper."""
    return ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def sync(what=None):
    """Wait for a stream (or the device). A HIP error ends the session: nothing more is launched on a device
    that has faulted."""
    try:
        (what or torch.cuda).synchronize()
    except RuntimeError as ex:
        pytest.exit(f"HIP error, stopping the session: {ex}", returncode=3)


def ok(rc, name):
    if rc == EHIP:
        from clasfv_amd import _lib
        pytest.exit(f"{name}: HIP error {_lib.load().clasfv_last_error()}, stopping the session", returncode=3)
    if rc != 0:
        from clasfv_amd import _lib
        raise AssertionError(f"{name} refused the call ({rc}): {_lib.load().clasfv_last_error()}")


def sleep_rate():
    """Cycles of torch.cuda._sleep per second, measured once with two events (the unit is not the shader
    clock): the sleep is lengthened until it takes 20 ms, so that launch overhead is under a percent."""
    if "rate" not in _state:
        s = torch.cuda.current_stream(dev())
        cycles = 1_000_000
        torch.cuda._sleep(1000)  # loads the kernel
        sync(s)
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record()
                torch.cuda._sleep(cycles)
                e1.record()
            sync(s)
            ms = e0.elapsed_time(e1)
            if ms >= 20.0 or cycles >= 10 ** 11:
                break
            cycles = int(cycles * max(2.0, 30.0 / max(ms, 1e-3)))
        assert ms >= 20.0, f"torch.cuda._sleep({cycles}) took {ms} ms: cannot calibrate the blocker"
        _state["rate"] = cycles / (ms * 1e-3)
        print(f"STREAM_BLOCKER calibration: {cycles} cycles in {ms:.2f} ms, {_state['rate']:.4e} cycles/s")
    return _state["rate"]


class Blocker:
    """Finite device work on ``stream``: one sleep kernel of ``seconds``, between two events."""

    def __init__(self, stream, seconds):
        self.seconds = seconds
        self.begin, self.done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles = int(seconds * sleep_rate())
        with torch.cuda.stream(stream):
            self.begin.record()
            torch.cuda._sleep(cycles)
            self.done.record()

    def running(self):
        return not self.done.query()

    def measured(self):
        """Seconds the sleep took (after it has finished)."""
        return self.begin.elapsed_time(self.done) * 1e-3


def block_seconds(t_host):
    return min(MAX_BLOCK, max(MIN_BLOCK, HOST_FACTOR * t_host))


# ---- bits --------------------------------------------------------------------------------------------
def bits(t):
    assert t.is_contiguous()
    return t.detach().reshape(-1).view(_INT[t.element_size()])


def sentinel_of(t):
    return SENTINEL_U8 if t.element_size() == 1 else -1


def put_sentinel(t):
    bits(t).fill_(sentinel_of(t))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def bar_units(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|)."""
    g, w = got.detach().double(), want.detach().double()
    return float(((g - w).abs() / (atol + rtol * w.abs())).max())


# ---- one call ------------------------------------------------------------------------------------------
class Case:
    """One call under test.

    call()      issues it on the current stream and returns its result tensors (the preallocated outputs, the
                buffers it changes in place, or what a Python wrapper allocated);
    bufs        the device buffers it reads, real / stale the staged inputs A / A' of the same shapes;
    outs        preallocated outputs (sentinel-filled before every run);
    close       {result index: (rtol, atol)}: results whose float atomics take another order every run; they
                are within the bar of R(A) and farther than it from R(A');
    between()   more work enqueued on the stream between the input copies and the call;
    settled()   called after every synchronisation (for state the call accumulates);
    kernels     the __global__ functions or conv kernel names the call launches (coverage tables)."""

    def __init__(self, name, call, bufs=(), real=(), stale=(), outs=(), close=None, between=None, settled=None,
                 kernels=()):
        assert len(bufs) == len(real) == len(stale)
        for b, a, s in zip(bufs, real, stale):
            assert b.shape == a.shape == s.shape and b.dtype == a.dtype == s.dtype, name
        self.name, self.call, self.bufs, self.real, self.stale = name, call, list(bufs), list(real), list(stale)
        self.outs, self.close, self.between, self.settled = list(outs), dict(close or {}), between, settled
        self.kernels = set(kernels)

    def load(self, which):
        """Copies on the current stream."""
        with torch.no_grad():
            for b, src in zip(self.bufs, which):
                b.copy_(src)

    def reset(self, which):
        self.load(which)
        for o in self.outs:
            put_sentinel(o)

    def settle(self, what=None):
        sync(what)
        if self.settled:
            self.settled()

    def serial(self, which):
        """R(which) on the default stream, fully synchronised; clones, which nothing changes afterwards."""
        self.reset(which)
        sync()
        res = self.call()
        self.settle()
        return [r.detach().clone() for r in res]

    def references(self):
        ref, stale_ref = self.serial(self.real), self.serial(self.stale)
        assert len(ref) == len(stale_ref) and ref
        for i, (a, b) in enumerate(zip(ref, stale_ref)):
            assert bool((bits(a) != sentinel_of(a)).any()), f"{self.name}: result {i} was not written"
            if i in self.close:
                assert bar_units(b, a, *self.close[i]) > 1.0, f"{self.name}: result {i} of A' is within the bar of A's"
            else:
                assert not same_bits(a, b), f"{self.name}: result {i} is the same for A and A': the case tells nothing"
        return ref, stale_ref

    def warm(self, stream):
        """Every per-call cost on ``stream`` paid (context, arena, function attributes, cached tables), then
        the host time of one call on the idle stream."""
        with torch.cuda.stream(stream):
            self.call()
            if self.between:
                self.between()
        self.settle(stream)
        with torch.cuda.stream(stream):
            t0 = time.perf_counter()
            self.call()
            t_host = time.perf_counter() - t0
        self.settle(stream)
        return t_host

    def compare(self, res, ref, stale_ref, who=""):
        assert len(res) == len(ref)
        for i, (g, a, b) in enumerate(zip(res, ref, stale_ref)):
            what = f"{self.name}{who}: result {i}"
            if i in self.close:
                da, db = bar_units(g, a, *self.close[i]), bar_units(g, b, *self.close[i])
                print(f"STREAM_BAR {what}: {da:.4g} bars (rtol {self.close[i][0]:.3g}, atol {self.close[i][1]:.3g}) from "
                      f"the serial result, {db:.4g} from the stale one")
                assert da <= 1.0, f"{what} is {da:.3g} bars from the serial result (and {db:.3g} from the stale one)"
                assert db > 1.0, f"{what} is within the bar of the stale result"
            else:
                assert g.shape == a.shape and g.dtype == a.dtype, what
                wrong = int((bits(g) != bits(a)).sum())
                assert wrong == 0, f"{what}: {wrong} of {a.numel()} elements differ from the serial result" + \
                    (" (it equals the stale result)" if same_bits(g, b) else "")


WAITED = ("the blocker had finished when the call returned: either the call waited for the device, or it took "
          "longer on the host than the blocker lasts ({seconds:.3f} s = max(0.25 s, 50 x the {t_host:.3e} s "
          "measured on the idle stream, at most 1 s)")


def run_behind_blocker(case, asynchronous=True):
    """The protocol of this module's docstring for one case; prints its STREAM_CASE line. ``asynchronous``
    False: the call is documented to wait for its stream, and only its results are checked."""
    s = side_streams()[0]
    ref, stale_ref = case.references()
    t_host = case.warm(s)
    case.reset(case.stale)
    sync()
    seconds = block_seconds(t_host)
    w0 = time.perf_counter()
    try:
        with torch.cuda.stream(s):
            blocker = Blocker(s, seconds)
            case.load(case.real)
            if case.between:
                case.between()
            res = case.call()
            running = blocker.running()
    finally:   # nothing stays queued behind the blocker, whatever the call raised
        sync(s)
    case.settle(s)
    wall = time.perf_counter() - w0
    print(f"STREAM_CASE {case.name} t_host_ms={t_host * 1e3:.3f} blocker_s={seconds:.3f} "
          f"blocker_measured_s={blocker.measured():.3f} wall_s={wall:.3f} returned_before_blocker_end={running}")
    if asynchronous:
        assert running, f"{case.name}: " + WAITED.format(seconds=seconds, t_host=t_host)
    case.compare(res, ref, stale_ref)
    return res


def overlaps(case_a, case_b, s1, s2, seconds=0.05):
    """One trial of the two-stream arrangement with a short blocker: does call B on ``s2`` complete on the
    device while call A sits behind the blocker on ``s1``? Both calls have been warmed on their streams."""
    case_a.reset(case_a.stale)
    case_b.reset(case_b.real)
    sync()
    try:
        with torch.cuda.stream(s1):
            blocker = Blocker(s1, seconds)
            case_a.load(case_a.real)
            case_a.call()
        with torch.cuda.stream(s2):
            case_b.call()
        sync(s2)
        beside = blocker.running()
    finally:
        sync()
    case_a.settle()
    case_b.settle()
    return beside


def run_two_streams(case_a, case_b, s1=None, s2=None):
    """Call A behind a blocker on ``s1``, call B (its inputs ready) on ``s2`` with none (by default the two
    side streams, which the runtime runs side by side). Both calls return while the blocker runs; B completes on
    the device and equals its serial result while A's blocker still runs; then A equals its serial result."""
    if s1 is None:
        s1, s2 = side_streams()
        assert streams_are_concurrent(), ("none of eight streams ran a kernel while a blocker held the first one: the "
                                          "runtime serialises them, and the two-stream cases can show nothing")
    b_on_null = s2.cuda_stream == 0
    ref_a, stale_a = case_a.references()
    ref_b, stale_b = case_b.references()
    t_host = case_a.warm(s1) + case_b.warm(s2)
    case_b.reset(case_b.real)
    sync()
    with torch.cuda.stream(s2):  # B's device time, to size the blocker
        t0 = time.perf_counter()
        case_b.call()
        sync(s2)
        t_b = time.perf_counter() - t0
    case_a.reset(case_a.stale)
    case_b.reset(case_b.real)
    sync()
    seconds = block_seconds(t_host + t_b)
    w0 = time.perf_counter()
    try:
        with torch.cuda.stream(s1):
            blocker = Blocker(s1, seconds)
            case_a.load(case_a.real)
            res_a = case_a.call()
            a_returned = blocker.running()
        with torch.cuda.stream(s2):
            res_b = case_b.call()
            b_returned = blocker.running()
        sync(s2)
        b_done = blocker.running()
        t_done = time.perf_counter() - w0
        case_b.compare(res_b, ref_b, stale_b, " (B)")
    finally:   # nothing stays queued behind the blocker, whatever failed
        sync(s1)
    case_a.settle(s1)
    wall = time.perf_counter() - w0
    print(f"STREAM_CASE two-streams {case_a.name} | {case_b.name}{' on the NULL stream' if b_on_null else ''} "
          f"t_host_ms={t_host * 1e3:.3f} b_ms={t_b * 1e3:.3f} blocker_s={seconds:.3f} "
          f"blocker_measured_s={blocker.measured():.3f} b_done_s={t_done:.3f} wall_s={wall:.3f} "
          f"a_returned_before_blocker_end={a_returned} b_returned_before_blocker_end={b_returned} "
          f"b_done_before_blocker_end={b_done}")
    assert a_returned, f"{case_a.name}: " + WAITED.format(seconds=seconds, t_host=t_host)
    assert b_returned, f"{case_b.name} (on the other stream): " + WAITED.format(seconds=seconds, t_host=t_host)
    assert b_done, (f"{case_b.name} on the other stream finished only after {case_a.name}'s blocker "
                    f"({seconds:.3f} s): it was ordered behind the other stream's work, or took that long")
    case_a.compare(res_a, ref_a, stale_a, " (A)")
