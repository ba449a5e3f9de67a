"""Time a chain of P warps on the GPU ("Tracking"):

  (a) warp_loop    P clasfv_warp launches, each reading the previous frame from HBM (what
                   apply_sequence_deformation and losses._propagate did before clasfv_track);
                   warp_loop_py is the same through warp.warp (one torch.empty_like per step), as
                   the package called it
  (b) track_lds    clasfv_track | CLASFV_TRACK_FORCE_LDS: one launch, the plane in LDS
  (c) track_steps  clasfv_track | CLASFV_TRACK_FORCE_STEPS: P launches of the step kernel
      track_auto   clasfv_track as callers get it (LDS up to CLASFV_TRACK_LDS_AUTO_PIXELS)

HIP events around REPS back-to-back chains on one stream (REPS / 2 in the sweep; windows of 0.1 to
0.7 s; the enqueue is part of what a caller waits for: a chain of tiny launches is bound by it); the
variants alternate over ROUNDS rounds after a warm-up of each, and the per-chain time of every round
is printed with the median. The outputs of the variants are compared bit for bit first. HBM bytes are computed from the shapes. The workload's
plane (112x112, N=4 C=2 and N=1 C=1, P=31) comes first, then a sweep of plane sizes that locates the
size below which one CU beats P launches.

    python tools/track_timing.py [--reps 2000] [--rounds 5]
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clasfv_amd import _lib, warp as W  # noqa: E402

T, P = 32, 31


def time_shape(lib, dev, N, C, H, Wd, reps, rounds, py_loop):
    rng = np.random.default_rng(5)
    img = torch.from_numpy(rng.uniform(0, 1, (N, C, H, Wd)).astype(np.float32)).to(dev)
    motion = torch.from_numpy(np.tanh(rng.normal(0, 0.15, (N, 4, T, H, Wd))).astype(np.float32)).to(dev)
    keys = ("warp_loop", "track_lds", "track_steps", "track_auto")
    out = {k: torch.empty((P, N, C, H, Wd), device=dev) for k in keys}
    stream = _lib.stream_ptr(device=dev)
    sn, sc, st = motion.stride(0), motion.stride(1), motion.stride(2)
    mptr = [ctypes.c_void_p(motion[:, :, t].data_ptr()) for t in range(T)]
    optr = {k: [ctypes.c_void_p(v[p].data_ptr()) for p in range(P)] for k, v in out.items()}

    def warp_loop():
        src = _lib.ptr(img)
        for p in range(P):
            _lib.check(lib.clasfv_warp(src, N, C, H, Wd, mptr[p], sn, sc, optr["warp_loop"][p], stream))
            src = optr["warp_loop"][p]

    def track(key, flag):
        def run():
            _lib.check(lib.clasfv_track(_lib.ptr(img), N, C, H, Wd, _lib.ptr(motion), sn, sc, st, T, 0, 1, P,
                                        _lib.TRACK_BILINEAR | flag, optr[key][0], stream))
        return run

    def loop_py():
        cur = img
        for t in range(P):
            cur = W.warp(cur, motion[:, 0:2, t])
        return cur

    variants = {"warp_loop": warp_loop, "track_lds": track("track_lds", _lib.TRACK_FORCE_LDS),
                "track_steps": track("track_steps", _lib.TRACK_FORCE_STEPS), "track_auto": track("track_auto", 0)}
    if py_loop:
        variants["warp_loop_py"] = loop_py
    for fn in variants.values():   # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    same = all(torch.equal(out["warp_loop"], out[k]) for k in keys[1:]) and torch.equal(loop_py(), out["track_lds"][-1])
    print(f"\nN={N} C={C} {H}x{Wd} ({H * Wd} pixels) P={P} bilinear: outputs of all variants bit-identical: {same}")
    assert same
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    hw4 = H * Wd * 4
    frame = N * C * hw4
    per_step = P * (2 * N * hw4 + 2 * frame)   # motion once per n, the previous frame read, the new one written
    on_chip = P * N * C * 2 * hw4 + frame + P * frame   # motion once per (n, c) plane, img read, every frame written
    auto_lds = H * Wd <= _lib.TRACK_LDS_AUTO_PIXELS
    moved = {"warp_loop": per_step, "warp_loop_py": per_step, "track_steps": per_step, "track_lds": on_chip,
             "track_auto": on_chip if auto_lds else per_step}
    for k, v in times.items():
        launches = 1 if k == "track_lds" or (k == "track_auto" and auto_lds) else P
        print(f"  {k:13s} median {statistics.median(v):8.1f} us/chain  (min {min(v):.1f}, max {max(v):.1f}; rounds: "
              f"{' '.join(f'{x:.1f}' for x in v)})  launches {launches}  HBM bytes {moved[k] / 1e6:.2f} MB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    print(f"device: {torch.cuda.get_device_name(0)}  reps per round: {args.reps} (sweep: {args.reps // 2})  "
          f"rounds: {args.rounds}  "
          f"CLASFV_TRACK_LDS_AUTO_PIXELS: {_lib.TRACK_LDS_AUTO_PIXELS}")
    for N, C in ((4, 2), (1, 1)):
        time_shape(lib, dev, N, C, 112, 112, args.reps, args.rounds, py_loop=True)
    print("\n---- plane-size sweep ----")
    for H, Wd in ((24, 20), (32, 40), (48, 48), (48, 64), (64, 64), (80, 80), (96, 96)):
        for N, C in ((4, 2), (1, 1)):
            time_shape(lib, dev, N, C, H, Wd, args.reps // 2, args.rounds, py_loop=False)


if __name__ == "__main__":
    main()
