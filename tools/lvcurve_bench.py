"""Time the LV curve on the GPU against the host EF stage it sits beside ("LV geometry"), on the
config[1] fused masks (200 x 112 x 112, tests/golden/northstar_c1.npz, device-resident), for one video and for
32 videos in one launch (the three northstar fixtures' masks in turn):

  (a) lv_curve     echo.lv_curve(masks).cpu(): from the launch to area, length, radii and volume on the host
                   (host clock around REPS calls, each ending in the copies' synchronisation)
  (b) kernel       clasfv_lv_geometry alone: HIP events around 5 * REPS back-to-back launches on one stream
  host EF          echo.compute_ef_using_putative_clips on the int64 masks: get2dPucks on the ED / ES frames only
                   (one thread per video; 32 videos through compute_ef_batch on 16 threads)
  host curve       the per-frame get2dPucks + _disk_volume loop, the only way to the curve without the kernel
                   (32 videos: one video per task on 16 threads)

Variants alternate over ROUNDS rounds after a warm-up; every round's time is printed with the median. The EFs
of the device curve are compared with the host's first. The bar: (a) for the whole 200-frame curve is shorter
than the host EF stage for its few frames.

    python tools/lvcurve_bench.py [--reps 1000] [--rounds 5]
"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clasfv_amd import _lib, echo  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
FIXTURES = ("northstar_c1.npz", "northstar_c1_random.npz", "northstar_c1_deep.npz")
CPUS = 16


def fused_masks(name):
    g = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    shp = tuple(int(x) for x in g["fused_simple_shape"])
    return np.unpackbits(g["fused_simple"])[: int(np.prod(shp))].reshape(shp).astype(np.int64)


def host_curve(masks):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array([echo._disk_volume(*echo.get2dPucks((m == 1).astype(int), (1.0, 1.0))) for m in masks])


def report(name, times, unit="us", note=""):
    scale = 1e6 if unit == "us" else 1e3
    v = [t * scale for t in times]
    print(f"  {name:12s} median {statistics.median(v):10.1f} {unit}  (min {min(v):.1f}, max {max(v):.1f}; rounds: "
          f"{' '.join(f'{x:.1f}' for x in v)}){note}")
    return statistics.median(times)


def bench(videos, dev, reps, rounds):
    """videos: list of (200,112,112) int64 host masks, timed as one (N,T,H,W) batch."""
    n = len(videos)
    host = np.stack(videos)
    masks = torch.from_numpy(host.astype(np.uint8)).to(dev)
    if n == 1:
        masks = masks[0]
    lib = _lib.load()
    f, (h, w) = masks.numel() // (masks.shape[-2] * masks.shape[-1]), masks.shape[-2:]
    area = torch.empty(f, dtype=torch.int32, device=dev)
    geom = torch.empty((f, _lib.LV_STRIDE), dtype=torch.float64, device=dev)
    stream = _lib.stream_ptr(device=dev)

    def curve():
        return echo.lv_curve(masks).cpu()

    def kernel():
        _lib.check(lib.clasfv_lv_geometry(_lib.ptr(masks), f, h, w, 1, 1.0, 1.0, _lib.ptr(area), _lib.ptr(geom), stream))

    pool = ThreadPoolExecutor(CPUS)

    def host_ef():
        if n == 1:
            return [echo.compute_ef_using_putative_clips(host[0], 0)]
        return echo.compute_ef_batch(list(host), workers=CPUS)

    def host_loop():
        return list(pool.map(host_curve, list(host)))

    for _ in range(5):  # warm-up: code object, allocator, LDS attribute
        c = curve()
        kernel()
    torch.cuda.synchronize()
    ref = host_ef()
    c_area, c_vol = c.area.reshape(n, -1), c.volume.reshape(n, -1)
    same = all(np.allclose(echo.ef_from_curve(c_area[i], c_vol[i], i), ref[i], rtol=0, atol=1e-6) for i in range(n))
    print(f"\n{n} video(s) x {host.shape[1]} frames of {h}x{w} ({f} frames in one launch, {masks.numel() / 1e6:.2f} MB "
          f"of masks): EFs from the device curve equal the host's within 1e-6: {same}")
    assert same
    t = {k: [] for k in ("lv_curve", "kernel", "host EF", "host curve")}
    host_reps = max(1, min(5, 40 // n))
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            curve()
        t["lv_curve"].append((time.perf_counter() - t0) / reps)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5 * reps):
            kernel()
        e1.record()
        e1.synchronize()
        t["kernel"].append(e0.elapsed_time(e1) * 1e-3 / (5 * reps))
        t0 = time.perf_counter()
        for _ in range(host_reps):
            host_ef()
        t["host EF"].append((time.perf_counter() - t0) / host_reps)
        t0 = time.perf_counter()
        host_loop()
        t["host curve"].append(time.perf_counter() - t0)
    a = report("(a) lv_curve", t["lv_curve"], note="  launch -> results on the host")
    b = report("(b) kernel", t["kernel"], note=f"  {statistics.median(t['kernel']) * 1e9 / f:.1f} ns per frame")
    ef = report("host EF", t["host EF"], "ms", f"  ED / ES frames only, {'1 thread' if n == 1 else f'{CPUS} threads'}")
    report("host curve", t["host curve"], "ms", f"  every frame, {'1 thread' if n == 1 else f'{CPUS} threads'}")
    print(f"  bar: (a) whole curve {a * 1e6:.1f} us < host EF stage {ef * 1e6:.1f} us: {a < ef}  "
          f"(host EF / (a) = {ef / a:.1f}x, kernel share of (a) {b / a:.0%})")
    pool.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    torch.set_num_threads(CPUS)
    print(f"device: {torch.cuda.get_device_name(0)}  host CPUs used: {CPUS}  reps per round: {args.reps}  "
          f"rounds: {args.rounds}")
    vids = [fused_masks(n) for n in FIXTURES]
    bench(vids[:1], dev, args.reps, args.rounds)
    bench([vids[i % 3] for i in range(32)], dev, max(1, args.reps // 4), args.rounds)


if __name__ == "__main__":
    main()
