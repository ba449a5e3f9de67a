"""Time beat tracking on the GPU ("Beat tracking") on the north-star video: T = 200 frames of 112 x 112
(synthetic.echo_video_uint8), synthetic weights, masks synthetic.ellipse_masks(200): beats (0,25), (50,75),
(100,125), (150,175), windows from frames 0, 47, 97, 147.

  track_beats    beats.track_beats with explicit pairs: windows, 4 beat clips, one forward, 8 chains, Dice, curves, EF
  forward        its beat-clip part alone: build_clips of the 4 windows + run_model(return_motion=True)
  chains         its 8 chains alone (beats.track_chains on the motion of that forward), as callers get them:
                 clasfv_track's own choice of path (the step kernel at this plane)
  chains_lds     the same with CLASFV_TRACK_FORCE_LDS (one launch per chain, the plane in LDS)
  segment        fuse_utils.segment_a_video_with_fusion_device(num_clips=5) on the same video: what a user
                 already pays before tracking

A host clock around REPS back-to-back calls that end in one device synchronise (the enqueue is part of what a
caller waits for); the variants alternate over ROUNDS rounds after a warm-up of each; every round is printed with
the median. The two chain variants are compared bit for bit first.

    python tools/beats_bench.py [--synthetic-weights SEED] [--reps 50] [--rounds 5]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clasfv_amd.synthetic as S  # noqa: E402
from clasfv_amd import _lib, beats, fuse_utils as FU, warp  # noqa: E402
from clasfv_amd.model import R2plus1D_18_MotionNet  # noqa: E402
from clasfv_amd.preprocess import preprocess_video  # noqa: E402
from clasfv_amd.weights import DEFAULT_SEED  # noqa: E402

T = 200
PAIRS = [(0, 25), (50, 75), (100, 125), (150, 175)]
STARTS = [0, 47, 97, 147]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic-weights", type=int, default=DEFAULT_SEED, metavar="SEED")
    ap.add_argument("--synthetic-recipe", choices=["echo", "random"], default="echo")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    model = R2plus1D_18_MotionNet(pretrained=False, seed=args.synthetic_weights, device=dev, weights=args.synthetic_recipe)
    video = preprocess_video(S.echo_video_uint8(T), 112, 112, device=dev)
    masks = torch.from_numpy(S.ellipse_masks(T)).to(dev, torch.uint8)
    assert [beats.beat_window(d, s, T)[0] for d, s in PAIRS] == STARTS
    found = beats.track_beats(video, masks, model)
    assert found.pairs == PAIRS and found.starts == STARTS and not found.skipped
    motion = FU.run_model(model, beats.beat_clips(video, STARTS), return_motion=True)[1]
    plain = dict(warp._MODES)
    forced = dict(plain, nearest=_lib.TRACK_NEAREST | _lib.TRACK_FORCE_LDS)

    def chains(modes):
        def run():
            warp._MODES.update(modes)
            try:
                return beats.track_chains(masks, motion, PAIRS, STARTS)
            finally:
                warp._MODES.update(plain)
        return run

    variants = {
        "track_beats": (lambda: beats.track_beats(video, masks, model, pairs=PAIRS), args.reps),
        "forward": (lambda: FU.run_model(model, beats.beat_clips(video, STARTS), return_motion=True), args.reps),
        "chains": (chains(plain), 4 * args.reps),
        "chains_lds": (chains(forced), 4 * args.reps),
        "segment": (lambda: FU.segment_a_video_with_fusion_device(video, model, num_clips=5), max(1, args.reps // 2)),
    }
    for fn, _ in variants.values():   # warm-up: code objects, allocator, the LDS attribute, the clip tables
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    a, b = variants["chains"][0](), variants["chains_lds"][0]()
    same = all(torch.equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
    steps = sum(es - ed for ed, es in PAIRS)
    print(f"device: {torch.cuda.get_device_name(0)}  video {tuple(video.shape)}  beats {PAIRS}  windows {STARTS}")
    print(f"8 chains of {steps // len(PAIRS)} steps each at 112x112, nearest: both paths bit-identical: {same}; tracked EF "
          f"(synthetic weights: no accuracy meant) seg {[round(x, 2) for x in found.ef_seg.tolist()]} forward "
          f"{[round(x, 2) for x in found.ef_forward.tolist()]}")
    assert same
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, (fn, reps) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / reps)
    med = {}
    for k, v in times.items():
        ms = [x * 1e3 for x in v]
        med[k] = statistics.median(ms)
        print(f"  {k:12s} median {med[k]:8.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}; {variants[k][1]} calls per round; "
              f"rounds: {' '.join(f'{x:.3f}' for x in ms)})")
    print(f"  track_beats / segment = {med['track_beats'] / med['segment']:.2f}; forward share of track_beats "
          f"{med['forward'] / med['track_beats']:.0%}; chains_lds / chains = {med['chains_lds'] / med['chains']:.2f}")


if __name__ == "__main__":
    main()
