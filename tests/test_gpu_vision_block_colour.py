"""GPU test of colour frames through the block-wise facade (CSLAM::SLAMBlockColour, CSLAM::blockOverlayAll; cslam_vision colour=2 / colour=1 with block=<F>,
overlays=<file>).

Sequence: tests/test_gpu_vision_block.py's — 24 frames of 640 x 480 rolled one pixel per frame under a robot that moves 1 cm per frame, min_matches=4 — built
from a colour base image whose B, G and R are three different textures (tests/test_gpu_unique.py's recipe, seeds CHANNEL_SEEDS); the file holds 3 bytes per pixel.
The seeds were chosen from runs of the step-wise colour route on the device: of (17, 18, 19), (17, 5, 9), (3, 17, 11), (1, 2, 3), (21, 22, 23) and (17, 29, 41) only
(21, 22, 23) keeps at least MIN_MATCHES matches in every frame behind the first (5 to 7; frame 0 creates the map and has nothing to match) — the others fall to
0 - 3 matches — and it runs 4 blocks, 2 of them full and 1 stopped early, with one deletion.
The gray file holds tests/np_overlay.gray of every frame: what loadPictures makes of it.

Compared, as text (every number is printed with %.17g, so equal lines are equal bits): colour=2 block=8 against block=8 on the gray file, and colour=2 block=1
against block=1 on the gray file — every "policy", "path", "frame", "ids" and "blocks" line.  Between the two routes (block=8 and block=1, both colour=2) two
kinds of line cannot be equal text by the tool's own definition: block=1 reports "blocks 0 ...", and a block prints "frame" and "ids" only for its last frame.
There: every "policy" and every "path" line equal as text (on this sequence the two routes' path rows are equal bits; tests/test_gpu_vision_block.py holds its own
sequence to 1e-9 / 1e-11), "frame" and "ids" equal for every frame the block route prints.  colour=1 block=8 prints what block=8 prints.
The overlays file: one frame per block-consumed frame, drawn on that frame's colour bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import np_overlay as OV
import test_gpu_detect as TD
from test_gpu_unique import _texture
from test_gpu_vision_block import BLOCK, FRAMES, MIN_MATCHES, ROLL, TOL_P, TOL_X, _report, _rows

pytestmark = pytest.mark.gpu

CHANNEL_SEEDS = (21, 22, 23)                                     # B, G, R
KINDS = ("policy", "path", "frame", "ids", "blocks")
W, H = 640, 480


def _lines(out, kinds=KINDS):
    return [ln for ln in out.splitlines() if ln.split() and ln.split()[0] in kinds]


def _run_colour(tmp, bgr, odo, *extra):
    """cslam_vision on a frames file of 3 bytes per pixel"""
    os.makedirs(tmp, exist_ok=True)
    with open(os.path.join(tmp, "frames.bin"), "wb") as f:
        f.write(struct.pack("iii", W, H, len(bgr)))
        for fr in bgr: f.write(np.ascontiguousarray(fr, dtype=np.uint8).tobytes())
    with open(os.path.join(tmp, "odo.txt"), "w") as f:
        for i, (x, y, th) in enumerate(odo): f.write(f"{i + 1} : {0.1 * i:.3f} {float(x)!r} {float(y)!r} {float(th)!r}\n")
    out = subprocess.run([TD.VISION, f"{tmp}/frames.bin", f"{tmp}/odo.txt", "colour=2", *extra], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def test_colour_frames_through_the_block_route(tmp_path):
    assert os.path.exists(TD.VISION), "run __graft_entry__.build() first"
    base = np.stack([_texture(np.random.default_rng(s)) for s in CHANNEL_SEEDS], axis=-1)
    assert base.shape == (H, W, 3) and (base[..., 0] != base[..., 1]).mean() > 0.5 and (base[..., 1] != base[..., 2]).mean() > 0.5
    bgr = [np.ascontiguousarray(np.roll(base, (0, ROLL * q), axis=(0, 1))) for q in range(FRAMES)]
    gray = [OV.gray(b) for b in bgr]
    odo = [(0.01 * i, 0.0, 0.0) for i in range(FRAMES + 1)]
    mm = f"min_matches={MIN_MATCHES}"
    t = str(tmp_path)
    c8 = _run_colour(t + "/c8", bgr, odo, f"block={BLOCK}", mm)
    c1 = _run_colour(t + "/c1", bgr, odo, "block=1", mm)
    os.makedirs(t + "/g8"); os.makedirs(t + "/g1"); os.makedirs(t + "/k8")
    g8 = TD._run_vision(t + "/g8", gray, odo, f"block={BLOCK}", mm)
    g1 = TD._run_vision(t + "/g1", gray, odo, "block=1", mm)
    k8 = TD._run_vision(t + "/k8", gray, odo, f"block={BLOCK}", mm, "colour=1")
    step, blk = _report(c1), _report(c8)
    matches = [int(r[-1]) for r in _rows(c1, "frame")]
    print("colour=2 block=1: matches", matches, "deleted", step["deleted"], "added", step["added"])
    print("colour=2 block=%d:" % BLOCK, blk["blocks"])
    # the run is not vacuous (the step-wise colour run alone, and the block counts)
    assert step["frames"] == list(range(FRAMES)) and len(matches) == FRAMES
    assert matches[0] == 0 and min(matches[1:]) >= MIN_MATCHES, matches      # (frame 0 creates the map: nothing to match yet)
    assert blk["blocks"]["blocks"] >= 2, blk["blocks"]
    # the same route on colour frames and on what loadPictures makes of them: the same text
    assert _lines(c8) == _lines(g8)
    assert _lines(c1) == _lines(g1)
    assert _lines(k8) == _lines(g8)
    # the two routes on colour frames
    assert _lines(c8, ("policy", "path")) == _lines(c1, ("policy", "path"))
    assert blk["frames"] == step["frames"] and blk["deleted"] == step["deleted"] and blk["added"] == step["added"]
    f8 = {ln.split()[1]: ln for ln in _lines(c8, ("frame",))}
    f1 = {ln.split()[1]: ln for ln in _lines(c1, ("frame",))}
    assert f8 and all(f1[k] == v for k, v in f8.items())
    assert sorted(blk["ids"]) and all(blk["ids"][f] == step["ids"][f] for f in blk["ids"])
    assert sorted(blk["path"]) == list(range(FRAMES)) == sorted(step["path"])
    dx = max(np.abs(blk["path"][f][:4] - step["path"][f][:4]).max() for f in blk["path"])
    dp = max(np.abs(blk["path"][f][4:] - step["path"][f][4:]).max() for f in blk["path"])
    print("path rows, block=%d against block=1 on colour frames: |dX| %.3e, |dP| %.3e, equal as text: %s" % (BLOCK, dx, dp, _lines(c8, ("path",)) == _lines(c1, ("path",))))
    assert dx <= TOL_X and dp <= TOL_P


def test_overlays_of_every_block_consumed_frame(tmp_path):
    assert os.path.exists(TD.VISION), "run __graft_entry__.build() first"
    base = np.stack([_texture(np.random.default_rng(s)) for s in CHANNEL_SEEDS], axis=-1)
    bgr = [np.ascontiguousarray(np.roll(base, (0, ROLL * q), axis=(0, 1))) for q in range(FRAMES)]
    odo = [(0.01 * i, 0.0, 0.0) for i in range(FRAMES + 1)]
    t = str(tmp_path)
    mm = f"min_matches={MIN_MATCHES}"
    plain = _run_colour(t + "/p", bgr, odo, f"block={BLOCK}", mm, f"display={t}/p/display.txt")
    out = _run_colour(t + "/o", bgr, odo, f"block={BLOCK}", mm, f"display={t}/o/display.txt", f"overlays={t}/o/overlays.bin")
    assert [ln for ln in out.splitlines() if not ln.startswith(("overlay_frames", "block_frames"))] == [ln for ln in plain.splitlines() if not ln.startswith("block_frames")]
    assert open(f"{t}/o/display.txt").read() == open(f"{t}/p/display.txt").read()
    rep = _report(out)
    consumed = [int(v) for v in _rows(out, "overlay_frames")[0]]
    assert len(consumed) == FRAMES - rep["blocks"]["fallback"] and consumed == sorted(set(consumed)) and len(consumed) >= 2
    raw = np.fromfile(f"{t}/o/overlays.bin", dtype=np.uint8)
    assert raw.size == len(consumed) * 3 * W * H
    ov = raw.reshape(len(consumed), H, W, 3)
    red, blue = np.array([0, 0, 255], dtype=np.uint8), np.array([255, 0, 0], dtype=np.uint8)      # B, G, R of CV_RGB(255, 0, 0) and CV_RGB(0, 0, 255)
    for q, fr in enumerate(consumed):
        diff = int((ov[q] != bgr[fr]).sum())
        assert 0 < diff < 0.05 * ov[q].size, (fr, diff)
        painted = (ov[q] == red).all(axis=2) | (ov[q] == blue).all(axis=2)
        assert (ov[q][~painted] == bgr[fr][~painted]).all(), fr      # every unpainted pixel is the colour source's
