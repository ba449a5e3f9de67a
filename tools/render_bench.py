"""Time the annotated-video kernel ("Annotated video") at the reference's geometry: 200 frames of
673 x 553 x 3 bytes (223 MB) from a 112 x 112 video, the config[1] fused masks (tests/golden/northstar_c1.npz)
and their volume curve read in place from clasfv_lv_geometry's output.

  kernel    clasfv_render_annotated: HIP events around REPS back-to-back calls on one stream (each call is the
            one-workgroup min / max reduction and the frame kernel)
  memset    hipMemsetAsync of the same byte count into the same buffer, timed the same way in the same run: the
            write rate this box gives without the kernel under test -- the yardstick, no rate is fixed in advance
  frames    render.annotate_video(...).cpu(): from the call to the frames on the host (host clock)
  --cli     also the end-to-end wall time of ``motion_segment.py`` on a 200-frame synthetic video with
            ``-c binary`` and with ``-c binary,gif`` (each once, after one warm-up run of the first)

Kernel and memset alternate over ROUNDS rounds after a warm-up; every round's time is printed with the median.

    python tools/render_bench.py [--frames 200] [--size 553] [--reps 20] [--rounds 5] [--cli]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import clasfv_amd.synthetic as S  # noqa: E402
from clasfv_amd import _lib, echo, render  # noqa: E402
from clasfv_amd.preprocess import preprocess_video  # noqa: E402


def fused_masks(frames):
    g = np.load(os.path.join(REPO, "tests", "golden", "northstar_c1.npz"), allow_pickle=False)
    shp = tuple(int(x) for x in g["fused_simple_shape"])
    m = np.unpackbits(g["fused_simple"])[: int(np.prod(shp))].reshape(shp).astype(np.uint8)
    return np.concatenate([m] * (-(-frames // len(m))))[:frames]


def hip_runtime():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = ctypes.CDLL(name)
        except OSError:
            continue
        hip.hipMemsetAsync.restype = ctypes.c_int
        hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
        return hip
    raise RuntimeError("libamdhip64.so not found: the memset yardstick needs the HIP runtime")


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def report(name, times, nbytes):
    us = [t * 1e6 for t in times]
    med = statistics.median(times)
    print(f"  {name:8s} median {med * 1e6:9.1f} us  {nbytes / med / 1e12:6.3f} TB/s written  (min {min(us):.1f}, max "
          f"{max(us):.1f}; rounds: {' '.join(f'{x:.1f}' for x in us)})")
    return med


def time_cli(frames):
    with tempfile.TemporaryDirectory() as tmp:
        vid = os.path.join(tmp, "clip.npy")
        np.save(vid, S.echo_video_uint8(frames, seed=7))
        out = {}
        for key, content in (("warm-up", "binary"), ("binary", "binary"), ("binary,gif", "binary,gif")):
            d = os.path.join(tmp, key.replace(",", "_"))
            os.mkdir(d)
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, os.path.join(REPO, "motion_segment.py"), "-p", vid, "--synthetic-weights",
                                "1234", "-f", "1", "--no-strict-reference", "-c", content, "-o", d],
                               capture_output=True, text=True, cwd=REPO)
            out[key] = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-2000:]
            size = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
            print(f"  motion_segment.py -c {content:11s} {out[key]:7.2f} s wall ({key}; {len(os.listdir(d))} files, "
                  f"{size / 1e6:.1f} MB)")
        print(f"  the gif keyword adds {out['binary,gif'] - out['binary']:.2f} s end to end (render, copy to the host, "
              f"PIL's GIF encoder)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--size", type=int, default=553)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cli", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    T, wo = args.frames, args.size
    hp, ht, hs = wo, render.TITLE_HEIGHT, render.STRIP_HEIGHT
    video = preprocess_video(S.echo_video_uint8(T, seed=1), 112, 112, device=dev)
    masks = torch.from_numpy(fused_masks(T)).to(dev)
    geom = echo.lv_curve(masks).geom
    band = torch.from_numpy(render.title_band(ht, wo)).to(dev)
    lib, hip = _lib.load(), hip_runtime()
    out = torch.empty((T, hp + ht + hs, wo, 3), dtype=torch.uint8, device=dev)
    work = torch.empty(lib.clasfv_render_workspace_bytes() // 8, dtype=torch.float64, device=dev)
    nbytes = out.numel()
    stream = _lib.stream_ptr(device=dev)
    vptr = ctypes.c_void_p(geom.data_ptr() + 8 * (_lib.LV_STRIDE - 1))

    def kernel():
        _lib.check(lib.clasfv_render_annotated(_lib.ptr(video), _lib.ptr(masks), None, T, 112, 112, vptr, _lib.LV_STRIDE,
                                               _lib.ptr(band), 0, T, hp, wo, ht, hs, 1, render.THICKNESS, _lib.ptr(work),
                                               _lib.ptr(out), stream), "clasfv_render_annotated")

    def memset():
        assert hip.hipMemsetAsync(_lib.ptr(out), 0, nbytes, stream) == 0

    def frames():
        return render.annotate_video(video, masks).cpu()

    print(f"device: {torch.cuda.get_device_name(0)}  {T} frames of {hp + ht + hs} x {wo} x 3 = {nbytes / 1e6:.1f} MB per "
          f"call  reps per round: {args.reps}  rounds: {args.rounds}")
    for _ in range(3):
        memset()
        kernel()
    torch.cuda.synchronize()
    ref = out.clone()
    assert torch.equal(frames().to(dev), ref), "annotate_video differs from the ABI call"
    t = {"kernel": [], "memset": [], "frames": []}
    for _ in range(args.rounds):
        t["memset"].append(events(memset, args.reps))
        t["kernel"].append(events(kernel, args.reps))
        t0 = time.perf_counter()
        frames()
        t["frames"].append(time.perf_counter() - t0)
    assert torch.equal(out, ref)
    k = report("kernel", t["kernel"], nbytes)
    m = report("memset", t["memset"], nbytes)
    print(f"  kernel / memset time = {k / m:.2f}  (the kernel writes at {m / k:.0%} of the memset's rate)")
    ms = [x * 1e3 for x in t["frames"]]
    print(f"  frames   median {statistics.median(ms):9.1f} ms  annotate_video(...).cpu(): volume curve, render and the copy "
          f"of {nbytes / 1e6:.0f} MB to pageable host memory  (rounds: {' '.join(f'{x:.1f}' for x in ms)})")
    if args.cli:
        time_cli(T)


if __name__ == "__main__":
    main()
