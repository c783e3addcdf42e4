"""GPU test of the block-wise facade with the state kept at a block's stop (CSLAM::resumeStoppedBlocks through cslam_vision block=8 resume=1)
against the same tool with block=8 alone, which rewinds a stopped block and runs the frames in front of the stop again.

Sequences: tests/test_gpu_vision_block.py's 24 frames (the map policy stops blocks) and tests/test_gpu_vision_block_ransac.py's with ransac=6 (a frame whose
consensus dropped a match stops blocks too).  Every "policy", "ransac" and "path" line must be EQUAL as text (the path rows are printed with %.17g: equal bits);
the timing line and the resumed= field are not compared.  resumed >= 1 in both runs: the path under test ran."""
import os
import re

import numpy as np
import pytest

import test_gpu_detect as TD
from test_gpu_unique import _texture
from test_gpu_vision_block import BLOCK, FRAMES, MIN_MATCHES, ROLL
from test_gpu_vision_block_ransac import HALF, LM_PX, SHIFT, SHIFT_FROM, THR

pytestmark = pytest.mark.gpu

KEYS = ("policy", "ransac", "path", "frame", "ids")


def _lines(out):
    return [ln for ln in out.splitlines() if ln.split() and ln.split()[0] in KEYS]


def _blocks(out):
    ln = [ln for ln in out.splitlines() if ln.startswith("blocks ")]
    assert len(ln) == 1, ln
    m = re.search(r"\bresumed=(\d+)\s*$", ln[0])
    return re.sub(r"\s*\bresumed=\d+\s*$", "", ln[0]), (int(m.group(1)) if m else None)


def _compare(tmp_path, frames, *args):
    odo = [(0.01 * i, 0.0, 0.0) for i in range(FRAMES + 1)]
    d0, d1 = tmp_path / "rerun", tmp_path / "resume"
    d0.mkdir(); d1.mkdir()
    out0 = TD._run_vision(str(d0), frames, odo, f"block={BLOCK}", f"min_matches={MIN_MATCHES}", *args)
    out1 = TD._run_vision(str(d1), frames, odo, f"block={BLOCK}", "resume=1", f"min_matches={MIN_MATCHES}", *args)
    b0, r0 = _blocks(out0)
    b1, r1 = _blocks(out1)
    print("rerun:", b0, "| resume:", b1, "resumed", r1, [ln for ln in (out0 + out1).splitlines() if ln.startswith("block_frames")])
    assert r0 is None                                            # without resume=1 the line is what it was
    l0, l1 = _lines(out0), _lines(out1)
    assert len([ln for ln in l0 if ln.startswith("path ")]) == FRAMES
    assert l1 == l0, [(a, b) for a, b in zip(l0, l1) if a != b][:3]
    assert b1 == b0
    assert r1 is not None and r1 >= 1, r1
    return out1


def test_policy_stops_resume_to_the_reruns_lines(tmp_path):
    assert os.path.exists(TD.VISION), "run __graft_entry__.build() first"
    base = _texture(np.random.default_rng(17))
    frames = [np.roll(base, (0, ROLL * q), axis=(0, 1)) for q in range(FRAMES)]
    _compare(tmp_path, frames)


def test_outlier_stops_resume_to_the_reruns_lines(tmp_path):
    assert os.path.exists(TD.VISION), "run __graft_entry__.build() first"
    base = _texture(np.random.default_rng(17))
    frames = []
    for q in range(FRAMES):
        fr = np.roll(base, (0, ROLL * q), axis=(0, 1))
        if q >= SHIFT_FROM:
            x, y = LM_PX[0] + ROLL * q, LM_PX[1]
            src = fr[y - HALF:y + HALF + 1, x - HALF:x + HALF + 1].copy()
            fr = fr.copy()
            fr[y - HALF + SHIFT[1]:y + HALF + 1 + SHIFT[1], x - HALF + SHIFT[0]:x + HALF + 1 + SHIFT[0]] = src
        frames.append(fr)
    out = _compare(tmp_path, frames, f"ransac={THR}")
    assert any(ln.startswith("ransac ") for ln in out.splitlines())
