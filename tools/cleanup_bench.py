"""Time label fusion with and without CLASFV_FUSE_CLEAN ("Mask cleanup") on the config[1] pass labels
(5 passes x 200 frames of 112 x 112, tests/golden/northstar_c1.npz, device-resident), per fusion method:

  plain     clasfv_fuse_votes(method): what the call launched before the flag existed
  clean     clasfv_fuse_votes(method | CLASFV_FUSE_CLEAN): the same launch and the cleanup launch behind it
  speckled  the flagged call on the same labels with islands and holes planted in every pass, so that every frame
            has several components, a hole to fill, and on every fourth frame a ring that makes a second candidate

and the cleanup alone (K = 1 majority, which copies the frame): the fused masks, a one-pixel-wide spiral filling
112 x 112 and 224 x 224 (one frame, and 200 of them), and sparse noise (many candidates, a flood for each).
HIP events around REPS back-to-back calls on one stream; the variants alternate over ROUNDS rounds after a warm-up
and every round's time is printed with the median. The cleaned frames are checked against tests/cleanup_oracle.py
first.

    python tools/cleanup_bench.py [--reps 200] [--rounds 5]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from clasfv_amd import _lib  # noqa: E402
from tests import cleanup_oracle as O  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
METHODS = {"majority": _lib.FUSE_MAJORITY, "itkvoting": _lib.FUSE_ITKVOTING, "simple": _lib.FUSE_SIMPLE,
           "staple": _lib.FUSE_STAPLE}
H = W = 112


def pass_labels():
    g = np.load(os.path.join(GOLDEN, "northstar_c1.npz"), allow_pickle=False)
    frames, t = [int(x) for x in g["pass_frames"]], int(g["T"])
    bits = np.unpackbits(g["passes"])[: sum(frames) * H * W].reshape(-1, H, W)
    lab, at = np.zeros((len(frames), t, H, W), np.uint8), 0
    for k, n in enumerate(frames):
        lab[k, :n] = bits[at:at + n]
        at += n
    return lab


def speckle(lab):
    out = lab.copy()
    out[:, :, 3:6, 4:9] = 1                    # islands, in every pass so that they survive the vote
    out[:, ::2, 100:104, 100:103] = 1
    out[:, :, 104, 8] = 1
    out[:, ::4, 84:108, 4:28] = 1              # a ring whose filled area rivals the LV's: a second candidate
    out[:, ::4, 85:107, 5:27] = 0
    members = lab[0].reshape(lab.shape[1], -1).argmax(axis=1)   # a hole at the first LV pixel of pass 0, one row down
    for f, p in enumerate(members):
        i, j = divmod(int(p), W)
        out[:, f, min(i + 2, H - 1), j] = 0
    return out


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def report(name, times, note=""):
    v = [t * 1e6 for t in times]
    print(f"  {name:34s} median {statistics.median(v):9.1f} us  (min {min(v):.1f}, max {max(v):.1f}; rounds: "
          f"{' '.join(f'{x:.1f}' for x in v)}){note}")
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lib, stream = _lib.load(), _lib.stream_ptr(device=dev)
    clean = _lib.clean_bits(128)
    print(f"device: {torch.cuda.get_device_name(0)}  reps per round: {args.reps}  rounds: {args.rounds}")

    def caller(labels, method):
        k, t, h, w = labels.shape
        out = torch.empty((t, h, w), dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.clasfv_fuse_votes(_lib.ptr(labels), k, t, 1, h, w, method, _lib.ptr(out), stream))
        call.out = out
        return call

    host = pass_labels()
    lab, spk = torch.from_numpy(host).to(dev), torch.from_numpy(speckle(host)).to(dev)
    print(f"\nfusion of {tuple(lab.shape)} pass labels, step 1 (the step it is added to takes about 21 ms)")
    for name, m in METHODS.items():
        calls = {"plain": caller(lab, m), "clean": caller(lab, m | clean), "speckled, clean": caller(spk, m | clean),
                 "speckled, plain": caller(spk, m)}
        for c in calls.values():
            c()
        torch.cuda.synchronize()
        for a, b in (("plain", "clean"), ("speckled, plain", "speckled, clean")):
            fused, got = calls[a].out.cpu().numpy(), calls[b].out.cpu().numpy()
            assert np.array_equal(got, O.clean_video(fused, 128)), (name, b)
            changed = int((got != fused).any(axis=(1, 2)).sum())
            print(f"  {name}: {b}: equals the oracle on all {len(got)} frames; {changed} frames changed")
        t = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, c in calls.items():
                t[k].append(timed(c, args.reps))
        med = {k: report(f"{name} {k}", v) for k, v in t.items()}
        print(f"  {name}: the flag adds {(med['clean'] - med['plain']) * 1e6:.1f} us on the fixture's masks, "
              f"{(med['speckled, clean'] - med['speckled, plain']) * 1e6:.1f} us on the speckled ones")

    print("\ncleanup alone (K = 1 majority copies the frames, then the cleanup launch)")
    r = np.random.default_rng(0)
    singles = {"spiral 112x112, 1 frame": O.spiral(112, 112)[None], "spiral 224x224, 1 frame": O.spiral(224, 224)[None],
               "spiral 112x112, 200 frames": np.repeat(O.spiral(112, 112)[None], 200, 0),
               "noise 0.33 112x112, 1 frame": (r.random((1, 112, 112)) < 0.33).astype(np.uint8),
               "noise 0.33 224x224, 1 frame": (r.random((1, 224, 224)) < 0.33).astype(np.uint8),
               "solid 224x224, 1 frame": np.ones((1, 224, 224), np.uint8)}
    calls = {}
    for name, frames in singles.items():
        x = torch.from_numpy(frames).to(dev)[None]
        calls[name] = caller(x, clean)
        calls[name + ", copy only"] = caller(x, 0)
        calls[name]()
        torch.cuda.synchronize()
        assert np.array_equal(calls[name].out[:1].cpu().numpy(), O.clean_video(frames[:1], 128)), name
    t = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, c in calls.items():
            t[k].append(timed(c, args.reps))
    for k, v in t.items():
        report(k, v)


if __name__ == "__main__":
    main()
