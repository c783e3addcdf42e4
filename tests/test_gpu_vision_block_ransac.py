"""GPU test of the block-wise facade with 1-point RANSAC (CSLAM::SLAMBlock with isUseRANSAC through cslam_vision block=<F> ransac=<thr>): the same
sequence through block=8 and through block=1 (SLAM() per frame, the same report lines).

Sequence: tests/test_gpu_vision_block.py's (the smooth texture, seed 17, rolled one pixel per frame under a robot that moves 1 cm per frame, 24 frames, 640 x 480,
min_matches=4; the map is what the facade's own detection finds in frame 0), with the 61 x 61 neighbourhood of the landmark detected at (425, 260) pasted 6 px to the
right of where the roll puts it from frame 13 on.  Threshold 6 px.  Chosen from runs of the step-wise route on the device (two landmarks, four shifts, 6 and 8 px),
not with the oracle on the CPU: at 8 px no frame of any candidate drops a match (a match shifted by 6 px leaves the 8-px search window before it leaves the
threshold); at 6 px frames 1..10 are clean (4 low-innovation inliers each), and from frame 11 on the roll's own drift puts a match outside the threshold, the
shifted neighbourhood changes which from frame 13 on.  Asserted on the block=1 run alone, before any comparison: frames 1..8 are clean, and a later frame's
rescue takes a match back (high >= 1).
Compared: the "ransac" line, the deleted IDs and the additions of every frame, the map's IDs behind every frame the block route reports them for, every path row
within the project's bounds (equality expected).  The block route: a frame with high >= 1 can only have run through SLAM() (a block's frames have no rescue, their
high is 0), so equal "ransac" lines show that the block ended in front of it and SLAM() ran it with its rescue; at least one block ended early, at least one ran
all 8 frames."""
import os

import numpy as np
import pytest

import test_gpu_detect as TD
from test_gpu_unique import _texture
from test_gpu_vision_block import BLOCK, FRAMES, MIN_MATCHES, ROLL, TOL_P, TOL_X, _report, _rows

pytestmark = pytest.mark.gpu

THR, LM_PX, SHIFT_FROM, SHIFT, HALF = 6.0, (425, 260), 13, (6, 0), 30


def _ransac_rows(out):
    return [(int(r[1]), int(r[3])) for r in _rows(out, "ransac")]


def test_block_route_with_ransac_equals_the_stepwise_route(tmp_path):
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
    odo = [(0.01 * i, 0.0, 0.0) for i in range(FRAMES + 1)]
    d1, d8 = tmp_path / "step", tmp_path / "block"
    d1.mkdir(); d8.mkdir()
    args = (f"min_matches={MIN_MATCHES}", f"ransac={THR}")
    out1 = TD._run_vision(str(d1), frames, odo, "block=1", *args)
    step, rs1 = _report(out1), _ransac_rows(out1)
    out8 = TD._run_vision(str(d8), frames, odo, f"block={BLOCK}", *args)
    blk, rs8 = _report(out8), _ransac_rows(out8)
    print("step-wise: ransac (low, high)", rs1, "deleted", step["deleted"], "added", step["added"])
    print("block-wise:", blk["blocks"], [ln for ln in (out1 + out8).splitlines() if ln.startswith("block_frames")])
    # the sequence does what it was chosen for (the reference run alone)
    assert step["frames"] == list(range(FRAMES)) and len(rs1) == FRAMES
    assert all(lo >= 2 and hi == 0 for lo, hi in rs1[1:BLOCK + 1])                # a block's worth of clean frames behind frame 0
    rescued = [f for f, (lo, hi) in enumerate(rs1) if hi >= 1]
    assert rescued and rescued[0] > BLOCK, rescued
    # the comparison
    assert blk["frames"] == step["frames"]
    assert rs8 == rs1
    assert blk["deleted"] == step["deleted"] and blk["added"] == step["added"]
    assert sorted(blk["ids"]) and all(blk["ids"][f] == step["ids"][f] for f in blk["ids"])
    assert blk["ids"][FRAMES - 1] == step["ids"][FRAMES - 1]
    dx = max(np.abs(blk["path"][f][:4] - step["path"][f][:4]).max() for f in blk["path"])
    dp = max(np.abs(blk["path"][f][4:] - step["path"][f][4:]).max() for f in blk["path"])
    print("path rows compared: %d, |dX| %.3e, |dP| %.3e; frames whose rescue took a match: %s" % (len(blk["path"]), dx, dp, rescued))
    assert dx <= TOL_X and dp <= TOL_P
    assert sorted(blk["path"]) == list(range(FRAMES)) == sorted(step["path"])
    assert blk["blocks"]["early"] >= 1 and blk["blocks"]["full"] >= 1, blk["blocks"]
    assert blk["blocks"]["fallback"] >= 1 + len(rescued), blk["blocks"]          # frame 0 and every frame that needed SLAM()'s rescue
