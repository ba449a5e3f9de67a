"""Generate tests/golden/overlay.npz by running the REFERENCE's echonet_overlay.

Imports /root/reference/src/visualization_utils.py with the stubs of make_golden_track.py (matplotlib and the
echo utilities stay inert: nothing is plotted). As make_annotated_gif does (:476-483), the gray video is
``np.dot(video.transpose([1, 2, 3, 0]), [.2989, .5870, .1140])``; each frame then goes through
``echonet_overlay(gray, seg, vis=False)`` (the overlay I) and through
``echonet_overlay(gray, seg, lab_gt=gt, vis=True, return_overlay=True)`` (the difference image I_gt, returned
before any plotting). The float64 results are stored; the inputs are regenerated from the seed in the tests
(tests/render_oracle.py, ``overlay_inputs``).
Run: ``python tests/golden/make_golden_overlay.py [--out PATH]``.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True


def generate():
    from tests.golden.make_golden import REF, _stub, install_stubs
    from tests.render_oracle import overlay_inputs
    install_stubs()
    for name, attrs in (("matplotlib", {}), ("matplotlib.backends", {}),
                        ("matplotlib.backends.backend_agg", {"FigureCanvasAgg": None}),
                        ("matplotlib.figure", {"Figure": None}), ("matplotlib.pyplot", {}),
                        ("matplotlib.colors", {"ListedColormap": None}),
                        ("src.utils.echo_utils", {"makeVideo": None, "computeSimpsonVolume": None}),
                        ("src.utils.camus_validate", {"labColor_cmap": None, "labColorMap": None})):
        _stub(name, **attrs)
    sys.path.insert(0, REF)
    from src.visualization_utils import echonet_overlay
    d = overlay_inputs()
    gray_video = np.dot(d["video"].transpose([1, 2, 3, 0]), np.array([.2989, .5870, .1140]))
    overlay = np.stack([echonet_overlay(g, s, vis=False) for g, s in zip(gray_video, d["seg"])])
    diff = np.stack([echonet_overlay(g, s, lab_gt=t, vis=True, return_overlay=True)
                     for g, s, t in zip(gray_video, d["seg"], d["gt"])])
    assert overlay.dtype == diff.dtype == np.float64
    return dict(overlay=overlay, diff=diff)


def main():
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "overlay.npz")
    out = generate()
    np.savez(path, **out)
    print({k: (np.shape(v), float(np.sum(v))) for k, v in out.items()})


if __name__ == "__main__":
    main()
