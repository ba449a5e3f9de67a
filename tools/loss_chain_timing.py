"""Time losses.motion_seg_loss (forward + backward) with its label chains on warp.track against the form it
had before: one stacked warp.warp per frame for the ED- and ES-seeded chains of a direction
("Tracking"). Host clock around REPS loss evaluations that end in a device synchronise, the two
forms alternating over ROUNDS rounds after a warm-up; loss values are compared first (bit-identical forward).

    python tools/loss_chain_timing.py [--reps 30] [--rounds 5]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clasfv_amd import losses  # noqa: E402
from clasfv_amd.warp import warp  # noqa: E402


def stacked_loop_propagate(seeds, motion, direction, start, end):
    """losses._propagate before warp.track: chains active at the same frame share one warp launch."""
    fields = motion[:, 0:2] if direction > 0 else motion[:, 2:4]
    n = fields.shape[0]
    frames = {k: f for k, (f, _) in seeds.items()}
    state = {k: lab for k, (_, lab) in seeds.items()}
    out = {k: [] for k in seeds}
    f = min(frames.values()) if direction > 0 else max(frames.values())
    while True:
        land = f + direction
        if (land >= end) if direction > 0 else (f <= start):
            break
        active = [k for k in seeds if (frames[k] <= f if direction > 0 else frames[k] >= f)]
        if active:
            moved = warp(torch.cat([state[k] for k in active]), fields[:, :, f].repeat(len(active), 1, 1, 1))
            for i, k in enumerate(active):
                state[k] = moved[i * n:(i + 1) * n]
                out[k].append((land, state[k]))
        f = land
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    forms = {"track": losses._propagate, "stacked_loop": stacked_loop_propagate}
    T, ed_i, es_i = 32, 4, 20
    print(f"device: {torch.cuda.get_device_name(0)}  reps per round: {args.reps}  rounds: {args.rounds}  "
          f"T={T} ed_index={ed_i} es_index={es_i}: chains of 27 + 11 (forward) and 20 + 4 (backward) steps")
    for N, H, W in ((1, 112, 112), (4, 112, 112), (1, 32, 40), (4, 32, 40)):
        rng = np.random.default_rng(3)
        yy, xx = np.mgrid[0:H, 0:W]
        r2 = (yy - H / 2) ** 2 + (xx - W / 2) ** 2
        ed, es = (np.broadcast_to((r2 <= (r * H) ** 2).astype(np.int64), (N, 1, H, W)).copy() for r in (0.3, 0.2))
        motion0 = torch.from_numpy(np.tanh(rng.normal(0, 0.15, (N, 4, T, H, W))).astype(np.float32)).to(dev)
        logits0 = torch.from_numpy(rng.normal(0, 1, (N, 2, T, H, W)).astype(np.float32)).to(dev)

        def run(form, backward=True):
            losses._propagate = forms[form]
            motion, logits = motion0.clone().requires_grad_(backward), logits0.clone().requires_grad_(backward)
            flow, ots = losses.motion_seg_loss(ed, es, ed_i, es_i, motion, torch.softmax(logits, 1), start=0, end=T)
            if backward:
                (flow + ots).backward()
            return float(flow), float(ots)

        try:
            vals = {k: run(k) for k in forms}
            for k in forms:   # warm-up
                run(k), run(k, False)
            torch.cuda.synchronize()
            times = {(k, b): [] for k in forms for b in (False, True)}
            for _ in range(args.rounds):
                for key in times:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        run(key[0], key[1])
                    torch.cuda.synchronize()
                    times[key].append((time.perf_counter() - t0) * 1e3 / args.reps)
        finally:
            losses._propagate = forms["track"]
        print(f"\nN={N} {H}x{W}: loss values track {vals['track']} stacked_loop {vals['stacked_loop']} "
              f"identical: {vals['track'] == vals['stacked_loop']}")
        for (k, b), v in times.items():
            print(f"  {k:13s} {'forward+backward' if b else 'forward only    '} median {statistics.median(v):7.2f} ms  "
                  f"(min {min(v):.2f}, max {max(v):.2f}; rounds: {' '.join(f'{x:.2f}' for x in v)})")


if __name__ == "__main__":
    main()
