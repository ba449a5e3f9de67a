"""Generate tests/golden/track.npz by running the REFERENCE's apply_sequence_deformation.

Imports /root/reference/src/visualization_utils.py with the stubs of make_golden.py plus inert ones
for what that module alone imports (matplotlib, src.utils.echo_utils, src.utils.camus_validate), on
torch CPU (``torch.Tensor.cuda`` patched to the identity: the reference's grid builder hard-codes
.cuda()). The reference returns only the last frame of a chain, so every intermediate frame is
recorded by calling it with a growing ``end_index``. Forward and backward chains over all T frames,
grid_mode "bilinear" on a float image and "nearest" on a label map. Inputs are regenerated from the
seed in tests (``track_inputs``); only the outputs are stored.
Run: ``python tests/golden/make_golden_track.py [--out PATH]``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

# (key, forward, start_index, grid_mode, input): end_index grows from start +- 1 to one past the last frame
CASES = [("fwd_bilinear", True, 0, "bilinear", "img"), ("bwd_bilinear", False, 5, "bilinear", "img"),
         ("fwd_nearest", True, 0, "nearest", "labels"), ("bwd_nearest", False, 5, "nearest", "labels")]


def track_inputs(N=2, C=2, T=6, H=24, W=20, seed=23):
    """Seeded inputs shared by this script and the tests. The flow reaches +-1.5 grid units (three
    quarters of the image), so chains clip at both borders; ``labels`` is a 4-class map as float32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    img = rng.uniform(0, 1, (N, C, H, W)).astype(np.float32)
    motion = (1.5 * np.tanh(rng.normal(0, 0.25, (N, 4, T, H, W)))).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.sqrt(((yy - H / 2) / (H / 2)) ** 2 + ((xx - W / 2) / (W / 2)) ** 2)
    rings = np.digitize(r, [0.3, 0.6, 0.9]).astype(np.float32)            # 0..3, concentric
    labels = np.stack([np.stack([np.roll(rings, (n, 2 * c), (0, 1)) for c in range(C)]) for n in range(N)])
    return dict(img=img, motion=motion, labels=labels, T=T)


def generate():
    from tests.golden.make_golden import REF, _stub, install_stubs
    install_stubs()
    for name, attrs in (("matplotlib", {}), ("matplotlib.backends", {}),
                        ("matplotlib.backends.backend_agg", {"FigureCanvasAgg": None}),
                        ("matplotlib.figure", {"Figure": None}), ("matplotlib.pyplot", {}),
                        ("matplotlib.colors", {"ListedColormap": None}),
                        ("src.utils.echo_utils", {"makeVideo": None, "computeSimpsonVolume": None}),
                        ("src.utils.camus_validate", {"labColor_cmap": None, "labColorMap": None})):
        _stub(name, **attrs)
    sys.path.insert(0, REF)
    torch.Tensor.cuda = lambda self, *a, **k: self
    from src.visualization_utils import apply_sequence_deformation
    d = track_inputs()
    motion = torch.from_numpy(d["motion"])
    out = {}
    for key, forward, start, mode, src in CASES:
        step = 1 if forward else -1
        frames = [apply_sequence_deformation(torch.from_numpy(d[src]), motion, start, start + step * (p + 1),
                                             grid_mode=mode, forward=forward).numpy()
                  for p in range(d["T"])]
        out[key] = np.stack(frames)
    return out


def main():
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "track.npz")
    out = generate()
    np.savez_compressed(path, **out)
    print({k: (np.shape(v), float(np.sum(v))) for k, v in out.items()})


if __name__ == "__main__":
    main()
