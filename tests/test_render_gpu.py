"""clasfv_render_annotated (csrc/render.hip) and its surface (render.annotate_video, the CLI's ``-c gif``).

The pane is pinned to the reference's echonet_overlay through tests/golden/overlay.npz, whole frames to
tests/render_oracle.py, the numpy restatement of the header's rules: every comparison is exact. The kernel is
called through the ctypes ABI with its output between guard bands, twice with different fill bytes: after a
launch the guards are intact, and the two outputs agree, so every output byte was written.
"""
import ctypes
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lvcurve_oracle as O
from tests import render_oracle as R
from tests import stream_order as SO
from tests.conftest import REPO, golden

pytestmark = pytest.mark.gpu

GUARD = 1024
EHIP = -4  # CLASFV_EHIP: the only return code after which the device may have faulted


def dev():
    return torch.device("cuda", 0)


def lib():
    from clasfv_amd import _lib
    return _lib.load()


def on_dev(a):
    return torch.as_tensor(a).to(dev()).contiguous()


def run_render(video, masks, volume=None, truth=None, title=None, first=0, count=None, Hp=None, Wo=None, Ht=0, Hs=0,
               label=1, thickness=2.0, offset=0, stride=1, stream=None, vol_dev=None):
    """Guarded clasfv_render_annotated calls -> (count, Hp + Ht + Hs, Wo, 3) numpy. ``offset`` bytes move out_dev
    off its allocation's alignment; ``stride`` spreads the volumes over a NaN-filled buffer; ``vol_dev`` =
    (tensor, first element, stride) reads them from a device tensor in place. A HIP error ends the session:
    nothing more is launched on a device that has faulted; a refusal, which never touches the device, fails."""
    from clasfv_amd import _lib
    video, masks = on_dev(video).float(), on_dev(masks).to(torch.uint8)
    _, T, H, W = video.shape
    Hp, Wo = H if Hp is None else Hp, W if Wo is None else Wo
    count = T - first if count is None else count
    truth = on_dev(truth).to(torch.uint8) if truth is not None else None
    title = on_dev(title).to(torch.uint8) if title is not None else None
    if vol_dev is None:
        vbuf = torch.full((T * stride,), float("nan"), dtype=torch.float64, device=dev())
        vbuf[::stride] = on_dev(np.asarray(volume, np.float64))
        vol_dev = (vbuf, 0, stride)
    vbuf, v0, vstride = vol_dev
    work = torch.full((lib().clasfv_render_workspace_bytes() // 8,), float("nan"), dtype=torch.float64, device=dev())
    total = count * (Hp + Ht + Hs) * Wo * 3
    got = []
    for fill in (0xA5, 0x5A):
        buf = torch.full((total + 2 * GUARD + 16,), fill, dtype=torch.uint8, device=dev())
        torch.cuda.synchronize()
        rc = lib().clasfv_render_annotated(
            _lib.ptr(video), _lib.ptr(masks), _lib.ptr(truth) if truth is not None else None, T, H, W,
            ctypes.c_void_p(vbuf.data_ptr() + 8 * v0), vstride, _lib.ptr(title) if title is not None else None,
            first, count, Hp, Wo, Ht, Hs, label, thickness, _lib.ptr(work),
            ctypes.c_void_p(buf.data_ptr() + GUARD + offset), _lib.stream_ptr(stream, dev()))
        if rc == EHIP:
            pytest.exit(f"clasfv_render_annotated: HIP error ({rc}) {lib().clasfv_last_error()}, stopping the session",
                        returncode=3)
        assert rc == 0, f"clasfv_render_annotated refused the call ({rc}): {lib().clasfv_last_error()}"
        try:
            torch.cuda.synchronize()
        except RuntimeError as ex:
            pytest.exit(f"clasfv_render_annotated: HIP error, stopping the session: {ex}", returncode=3)
        b = buf.cpu().numpy()
        lo, hi = GUARD + offset, GUARD + offset + total
        assert (b[:lo] == fill).all() and (b[hi:] == fill).all(), "write outside out"
        got.append(b[lo:hi].reshape(count, Hp + Ht + Hs, Wo, 3).copy())
    assert np.array_equal(got[0], got[1]), "output bytes left unwritten"
    return got[0]


def inputs(T, H, W, seed=5):
    """Seeded video in [0, 1] (an all-0 and an all-1 row), masks and truth of 0 / 1 / 2."""
    rng = np.random.default_rng(seed)
    video = rng.uniform(0, 1, (3, T, H, W)).astype(np.float32)
    video[:, :, 0], video[:, :, -1] = 0.0, 1.0
    return video, rng.integers(0, 3, (T, H, W)).astype(np.uint8), rng.integers(0, 3, (T, H, W)).astype(np.uint8)


def curve(T, kind="curve", seed=7):
    rng = np.random.default_rng(seed)
    k = np.arange(T, dtype=np.float64)
    v = 3000.0 + 1500.0 * np.sin(k / 3.0) + rng.normal(0, 40.0, T)
    if kind == "steep":
        v = 3000.0 + rng.uniform(-2500.0, 2500.0, T)
    elif kind == "const":
        v[:] = 1234.5
    elif kind == "nan_start":
        v[:max(1, T // 3)] = np.nan
    elif kind == "nan_mid":
        v[T // 2] = np.nan
        v[min(T - 1, T // 2 + 2)] = np.inf  # an infinite volume is no end point either
    elif kind == "nan_all":
        v[:] = np.nan
    elif kind == "one_finite":
        v[:] = np.nan
        v[T // 2] = 7.0
    return v


def title_image(Ht, Wo, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (Ht, Wo, 3)).astype(np.uint8)


def test_pane_equals_the_reference_overlay():
    """The pane at identity size against echonet_overlay run by the reference (overlay.npz): floor(255 * ref),
    exactly, on every pixel -- the fixture has no fragile pixel (255 * ref within 1e-9 of an integer while ref is
    neither 0 nor 1), which is asserted. The same for the difference image with ``truth``."""
    d, g = R.overlay_inputs(), golden("overlay.npz")
    for key, truth in (("overlay", None), ("diff", d["gt"])):
        ref = g[key]
        y = 255.0 * ref
        assert int(((np.abs(y - np.round(y)) < 1e-9) & (ref != 0) & (ref != 1)).sum()) == 0
        got = run_render(d["video"], d["seg"], np.zeros(4), truth=truth)
        assert got.shape == ref.shape
        wrong = int((got != np.floor(y).astype(np.uint8)).sum())
        assert wrong == 0, f"{key}: {wrong} of {got.size} bytes differ from floor(255 * reference)"


# name: T, H, W, then the call's keywords (curve kind under "kind", a title image under "with_title")
CASES = {
    # 3 * Wo = 33 bytes per row, 4785 bytes in all (1 mod 16); upscaled from a non-square source
    "up_nonsquare": (5, 7, 9, dict(Hp=20, Wo=11, Ht=3, Hs=6, with_title=True)),
    "out_off_by_1": (5, 7, 9, dict(Hp=20, Wo=11, Ht=3, Hs=6, with_title=True, offset=1)),
    "out_off_by_15": (5, 7, 9, dict(Hp=20, Wo=11, Ht=3, Hs=6, offset=15)),
    "down_with_truth": (4, 24, 40, dict(Hp=10, Wo=17, Ht=2, Hs=5, with_truth=True)),
    "up_x_down_y": (3, 24, 7, dict(Hp=10, Wo=20, Hs=4)),
    "T1": (1, 7, 9, dict(Hs=4)),
    "T2": (2, 7, 9, dict(Hs=4, Wo=10)),
    "many_samples_per_column": (70, 5, 6, dict(Hp=6, Wo=33, Hs=9, kind="steep")),
    "many_samples_thin": (70, 5, 6, dict(Hp=6, Wo=33, Hs=30, kind="steep", thickness=0.0)),
    "constant_curve": (6, 7, 9, dict(Hs=7, Wo=30, kind="const")),
    "nan_start": (9, 7, 9, dict(Hs=8, Wo=30, kind="nan_start")),
    "nan_middle": (9, 7, 9, dict(Hs=8, Wo=30, kind="nan_mid")),
    "nan_everywhere": (9, 7, 9, dict(Hs=8, Wo=30, kind="nan_all")),
    "one_finite_volume": (9, 7, 9, dict(Hs=8, Wo=30, kind="one_finite")),
    "no_title_no_strip": (3, 7, 9, dict(Hp=20, Wo=11)),
    "label_2": (3, 7, 9, dict(Hp=9, Wo=11, Hs=3, label=2, with_truth=True)),
    "thick_line": (8, 7, 9, dict(Hs=12, Wo=40, thickness=3.5)),
    "strided_volumes": (8, 7, 9, dict(Hs=12, Wo=40, stride=3)),
    "rows_of_48_bytes": (2, 7, 9, dict(Hp=4, Wo=16, Ht=1, Hs=3)),                  # every piece aligned, no tail
    "smaller_than_a_piece": (1, 3, 2, dict(Hp=1, Wo=2, Hs=1)),                     # 12 bytes: edge bytes only
    "smaller_than_a_piece_off_by_1": (1, 3, 2, dict(Hp=1, Wo=2, Hs=1, offset=1)),
    # the product geometry, and more 16-byte pieces (558,253) than one pass of the grid takes (524,288)
    "product_8_frames": (8, 112, 112, dict(Hp=553, Wo=553, Ht=40, Hs=80, with_title=True)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_full_frames_vs_oracle(name):
    """Whole frames against tests/render_oracle.py, exactly; mask pixels of value 2 lie beside the label's in
    every case."""
    T, H, W, kw = CASES[name]
    kw = dict(kw)
    video, masks, truth = inputs(T, H, W)
    volume = curve(T, kw.pop("kind", "curve"))
    Wo, Ht = kw.get("Wo", W), kw.get("Ht", 0)
    title = title_image(Ht, Wo) if kw.pop("with_title", False) else None
    truth = truth if kw.pop("with_truth", False) else None
    got = run_render(video, masks, volume, truth=truth, title=title, **kw)
    for k in ("offset", "stride"):
        kw.pop(k, None)
    want = R.render(video, masks, volume, truth=truth, title=title, **kw)
    assert got.shape == want.shape
    wrong = np.argwhere(got != want)
    assert len(wrong) == 0, f"{name}: {len(wrong)} of {got.size} bytes differ, first at (frame, row, col, ch) {wrong[0]}"
    if name == "product_8_frames":
        assert (got[-1, 593:] == R.LIME).all(axis=-1).any() and not got[0, 593:].any()  # a curve; none at frame 0


def test_chunks_and_single_frames_give_the_bytes_of_the_whole_call():
    """A frame depends on (T, i) and the inputs only: chunks [first, first + count) and single frames, at other
    output alignments, equal the slices of the whole call."""
    T, H, W = 7, 7, 9
    video, masks, truth = inputs(T, H, W, seed=9)
    volume = curve(T, "nan_mid")
    kw = dict(truth=truth, title=title_image(3, 11), Hp=20, Wo=11, Ht=3, Hs=6)
    whole = run_render(video, masks, volume, **kw)
    assert np.array_equal(whole, R.render(video, masks, volume, **kw))
    for first, count in ((0, 3), (3, 4), (2, 2), (6, 1)):
        part = run_render(video, masks, volume, first=first, count=count, offset=first, **kw)
        assert np.array_equal(part, whole[first:first + count]), (first, count)
    for i in range(T):
        assert np.array_equal(run_render(video, masks, volume, first=i, count=1, **kw)[0], whole[i]), i


def test_volumes_in_place_from_lv_geometry():
    """volume_dev = geom_dev + 11 with stride CLASFV_LV_STRIDE reads clasfv_lv_geometry's output where it lies."""
    from clasfv_amd import _lib, echo
    T, H, W = 12, 13, 29
    masks = O.ellipse_masks(H, W, count=T, seed=4).astype(np.uint8)
    masks[3] = 0  # an empty frame: volume 0
    video = inputs(T, H, W)[0]
    c = echo.lv_curve(on_dev(masks))
    volume = c.volume.cpu().numpy()
    assert np.isfinite(volume).sum() >= 6 and volume[3] == 0.0
    got = run_render(video, masks, Hp=20, Wo=45, Hs=16, vol_dev=(c.geom.view(-1), _lib.LV_STRIDE - 1, _lib.LV_STRIDE))
    assert np.array_equal(got, R.render(video, masks, volume, Hp=20, Wo=45, Hs=16))
    assert (got[-1, 20:] == R.LIME).all(axis=-1).any()


def test_behind_a_blocked_stream():
    """The call on a non-default stream whose head a sleep kernel holds, its inputs replaced behind the blocker:
    it returns before the blocker ends and equals the serial result of the real inputs, so both launches (the
    min / max reduction and the frames) and nothing else are ordered on the caller's stream."""
    from clasfv_amd import _lib
    T, H, W, Hp, Wo, Ht, Hs = 6, 7, 9, 20, 11, 3, 8
    real, stale = inputs(T, H, W, seed=1), inputs(T, H, W, seed=2)
    vols = [torch.from_numpy(curve(T, seed=s)).to(dev()) for s in (1, 2)]
    vols[1] = vols[1] * 3.0 + 500.0  # another range: a stale min / max moves the whole curve
    bufs = [torch.empty((3, T, H, W), device=dev()), torch.empty((T, H, W), dtype=torch.uint8, device=dev()),
            torch.empty((T,), dtype=torch.float64, device=dev())]
    title = on_dev(title_image(Ht, Wo))
    work = torch.zeros(lib().clasfv_render_workspace_bytes() // 8, dtype=torch.float64, device=dev())
    out = torch.empty((T, Hp + Ht + Hs, Wo, 3), dtype=torch.uint8, device=dev())

    def call():
        SO.ok(lib().clasfv_render_annotated(_lib.ptr(bufs[0]), _lib.ptr(bufs[1]), None, T, H, W, _lib.ptr(bufs[2]), 1,
                                            _lib.ptr(title), 0, T, Hp, Wo, Ht, Hs, 1, 2.0, _lib.ptr(work), _lib.ptr(out),
                                            SO.current_ptr()), "clasfv_render_annotated")
        return [out]

    case = SO.Case("render_annotated", call, bufs=bufs, real=[on_dev(real[0]), on_dev(real[1]), vols[0]],
                   stale=[on_dev(stale[0]), on_dev(stale[1]), vols[1]], outs=[out],
                   kernels=("render_minmax_kernel", "render_annotated_kernel"))
    res = SO.run_behind_blocker(case)
    want = R.render(real[0], real[1], vols[0].cpu().numpy(), Hp=Hp, Wo=Wo, Ht=Ht, Hs=Hs, title=title.cpu().numpy())
    assert np.array_equal(res[0].cpu().numpy(), want)
    src = open(os.path.join(REPO, "fully-automated-multi-heartbeat-echocardiography-video-segmentation-and-motion-"
                                  "tracking_amd", "csrc", "render.hip")).read()
    assert set(re.findall(r"__global__.*?void\s+(\w+)", src)) == case.kernels  # every kernel of render.hip ran here


@pytest.fixture(scope="module")
def echo_model():
    from clasfv_amd.model import R2plus1D_18_MotionNet
    return R2plus1D_18_MotionNet(pretrained=False, weights="echo")


def test_annotate_video_equals_the_abi_call(echo_model):
    """render.annotate_video on the fused masks of a 32-frame synthetic clip, at the reference's geometry: the
    bytes of the ABI call with the cached title band and lv_curve's volumes in place, which equal the oracle's;
    int64 masks, explicit volumes and chunks give the same bytes."""
    import clasfv_amd.synthetic as S
    from clasfv_amd import _lib, echo, render
    from clasfv_amd.fuse_utils import segment_a_video_with_fusion_device
    from clasfv_amd.preprocess import preprocess_video
    video = preprocess_video(S.echo_video_uint8(32, seed=7), 112, 112, device=dev())
    fused = segment_a_video_with_fusion_device(video, model=echo_model, num_clips=1, strict_reference=False)
    assert fused.dtype == torch.uint8 and fused.shape == (32, 112, 112) and bool(fused.any())
    frames = render.annotate_video(video, fused)
    assert frames.dtype == torch.uint8 and frames.is_cuda and frames.shape == (32, 553 + 40 + 80, 553, 3)
    c = echo.lv_curve(fused)
    band = render.title_band()
    got = run_render(video, fused, title=band, Hp=553, Wo=553, Ht=40, Hs=80, thickness=render.THICKNESS,
                     vol_dev=(c.geom.view(-1), _lib.LV_STRIDE - 1, _lib.LV_STRIDE))
    assert np.array_equal(frames.cpu().numpy(), got)
    want = R.render(video.cpu().numpy(), fused.cpu().numpy(), c.volume.cpu().numpy(), Hp=553, Wo=553, Ht=40, Hs=80,
                    thickness=render.THICKNESS, title=band)
    assert np.array_equal(got, want)
    assert (got[-1, 593:] == R.LIME).all(axis=-1).any() and (got[:, :553, :, 0] > got[:, :553, :, 2]).any()
    assert torch.equal(render.annotate_video(video, fused.to(torch.int64), volume=c.volume, first=5, count=3), frames[5:8])
    assert torch.equal(render.annotate_video(video, fused, volume=c.volume.cpu().numpy(), first=31), frames[31:])
    plain = render.annotate_video(video, fused, title=False, size=40, title_height=0, strip_height=0, first=0, count=2)
    assert np.array_equal(plain.cpu().numpy(), R.render(video.cpu().numpy(), fused.cpu().numpy(), np.zeros(32), count=2,
                                                        Hp=40, Wo=40))


def run_cli(out, content, vid, env=None):
    out.mkdir()
    r = subprocess.run([sys.executable, "motion_segment.py", "-p", str(vid), "--synthetic-weights", "1234", "-f", "1",
                        "--no-strict-reference", "-c", content, "-o", str(out)],
                       capture_output=True, text=True, timeout=180, cwd=REPO, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def cli_binary(tmp_path_factory):
    """The ``-c binary`` run both CLI tests compare with: (directory of the run, path of the video)."""
    import clasfv_amd.synthetic as S
    root = tmp_path_factory.mktemp("render_cli")
    vid = root / "clip32.npy"
    np.save(vid, S.echo_video_uint8(32, seed=7))
    run_cli(root / "binary", "binary", vid)
    return root / "binary", vid


def same_pickles(with_gif, binary, extra):
    names = sorted(os.listdir(binary))
    assert sorted(os.listdir(with_gif)) == sorted(names + extra)
    for f in names:
        assert (with_gif / f).read_bytes() == (binary / f).read_bytes(), f


@pytest.mark.timeout(400)
def test_cli_gif(cli_binary, tmp_path):
    """``-c binary,gif`` writes <name>_annotated.gif with one frame per video frame at the reference's size,
    without the old warning; the ``-c binary`` pickles are byte-identical with and without the keyword."""
    Image = pytest.importorskip("PIL.Image")
    binary, vid = cli_binary
    r = run_cli(tmp_path / "gif", "binary,gif", vid)
    assert "skipped" not in r.stderr and "warning" not in r.stderr
    same_pickles(tmp_path / "gif", binary, ["clip32_annotated.gif"])
    with Image.open(tmp_path / "gif" / "clip32_annotated.gif") as im:
        assert im.n_frames == 32 and im.size == (553, 553 + 40 + 80)
        assert im.info.get("loop") == 0


@pytest.mark.timeout(400)
def test_cli_gif_without_pil(cli_binary, tmp_path):
    """Where PIL does not import (here: a stand-in package that raises ImportError, first on the child's path),
    ``-c gif`` writes <name>_annotated.npy with a notice: annotate_video's bytes for the masks of
    ``-c binary_video``. The pickles stay byte-identical."""
    from clasfv_amd import render
    from clasfv_amd.preprocess import preprocess_video
    binary, vid = cli_binary
    (tmp_path / "nopil" / "PIL").mkdir(parents=True)
    (tmp_path / "nopil" / "PIL" / "__init__.py").write_text("raise ImportError('PIL is hidden from this run')\n")
    path = [str(tmp_path / "nopil")] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(path))
    r = run_cli(tmp_path / "npy", "binary,binary_video,gif", vid, env=env)
    assert "clip32_annotated.npy" in r.stderr and "skipped" not in r.stderr
    same_pickles(tmp_path / "npy", binary, ["clip32_annotated.npy", "clip32_whole_video_segmentation.pkl"])
    frames = np.load(tmp_path / "npy" / "clip32_annotated.npy")
    masks = pickle.load(open(tmp_path / "npy" / "clip32_whole_video_segmentation.pkl", "rb"))
    video = preprocess_video(np.load(vid), 112, 112, device=dev())
    want = render.annotate_video(video, torch.from_numpy(masks).to(dev()), title=False)
    assert frames.dtype == np.uint8 and frames.shape == (32, 673, 553, 3)
    assert np.array_equal(frames, want.cpu().numpy())
