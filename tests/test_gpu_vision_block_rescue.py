"""GPU test of the facade with the rescue gate on the device (CSLAM::rescueGateOnDevice through cslam_vision ransac=<thr> rescue=1): the
24-frame sequence of tests/test_gpu_vision_block_ransac.py at 6 px through block=8 rescue=1 and block=1 rescue=1 against block=1 without the gate.

What the sequence must show is asserted first, on the step-wise runs alone: at least one frame whose consensus dropped a match that the rescue did not take back
(block=1 rescue=1 counts them: every such frame saves its srukf_repredict_measurement, "gate_skips"), and at least one frame with a rescue (high >= 1).
Compared: the "ransac" line, the deleted IDs and the additions of every frame, the map's IDs, every path row within the block test's own bounds.  The block route
with the gate falls back to SLAM() for frame 0 and for every frame with a rescue, and no longer for the frames that only dropped matches; resume=1 on top prints
the same lines."""
import os

import numpy as np
import pytest

import test_gpu_detect as TD
from test_gpu_unique import _texture
from test_gpu_vision_block import BLOCK, FRAMES, MIN_MATCHES, ROLL, TOL_P, TOL_X, _report, _rows
from test_gpu_vision_block_ransac import HALF, LM_PX, SHIFT, SHIFT_FROM, THR, _ransac_rows

pytestmark = pytest.mark.gpu


def _frames():
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
    return frames


def _skips(out):
    t = [w for w in [ln for ln in out.splitlines() if ln.startswith("blocks ")][0].split() if w.startswith("gate_skips=")]
    return int(t[0].split("=")[1]) if t else None


def _lines(out):
    return [ln for ln in out.splitlines() if ln.split() and ln.split()[0] in ("policy", "frame", "ids", "ransac")]


def test_block_route_with_the_rescue_gate_equals_the_stepwise_route(tmp_path):
    assert os.path.exists(TD.VISION), "run __graft_entry__.build() first"
    frames = _frames()
    odo = [(0.01 * i, 0.0, 0.0) for i in range(FRAMES + 1)]
    args = (f"min_matches={MIN_MATCHES}", f"ransac={THR}")
    outs = {}
    for name, extra in (("step", ("block=1",)), ("step_gate", ("block=1", "rescue=1")), ("block_gate", (f"block={BLOCK}", "rescue=1")), ("block", (f"block={BLOCK}",)),
                        ("block_gate_resume", (f"block={BLOCK}", "rescue=1", "resume=1"))):
        d = tmp_path / name; d.mkdir()
        outs[name] = TD._run_vision(str(d), frames, odo, *extra, *args)
    rep = {k: _report(v) for k, v in outs.items()}
    rs = {k: _ransac_rows(v) for k, v in outs.items()}
    skips_step, skips_blk = _skips(outs["step_gate"]), _skips(outs["block_gate"])
    rescued = [f for f, (lo, hi) in enumerate(rs["step"]) if hi >= 1]
    print("step-wise: ransac (low, high)", rs["step"])
    print("frames with a rescue:", rescued, "| frames with a dropped match and no rescue (gate_skips, step-wise):", skips_step, "| in the block route's SLAM() frames:", skips_blk)
    for k in outs: print(k, rep[k]["blocks"], [ln for ln in outs[k].splitlines() if ln.startswith("block_frames")])
    # the sequence does what it is used for (the step-wise runs alone)
    assert rep["step"]["frames"] == list(range(FRAMES)) and len(rs["step"]) == FRAMES
    assert _skips(outs["step"]) is None and skips_step is not None and skips_step >= 1      # a frame with a dropped match and no rescue
    assert len(rescued) >= 1                                                                # and one with a rescue
    # the gate decides as the host's test does: the step-wise route prints the same lines with it
    assert _lines(outs["step_gate"]) == _lines(outs["step"])
    assert [ln for ln in outs["step_gate"].splitlines() if ln.startswith("path")] == [ln for ln in outs["step"].splitlines() if ln.startswith("path")]
    # the block route with the gate against the step-wise route without it
    for name in ("block_gate", "block_gate_resume"):
        blk, step = rep[name], rep["step"]
        assert blk["frames"] == step["frames"] and rs[name] == rs["step"], name
        assert blk["deleted"] == step["deleted"] and blk["added"] == step["added"], name
        assert sorted(blk["ids"]) and all(blk["ids"][f] == step["ids"][f] for f in blk["ids"]), name
        dx = max(np.abs(blk["path"][f][:4] - step["path"][f][:4]).max() for f in blk["path"])
        dp = max(np.abs(blk["path"][f][4:] - step["path"][f][4:]).max() for f in blk["path"])
        print("%s: path rows compared %d, |dX| %.3e, |dP| %.3e" % (name, len(blk["path"]), dx, dp))
        assert dx <= TOL_X and dp <= TOL_P, name
        assert sorted(blk["path"]) == list(range(FRAMES))
    assert _lines(outs["block_gate_resume"]) == _lines(outs["block_gate"])
    fb_on, fb_off = rep["block_gate"]["blocks"]["fallback"], rep["block"]["blocks"]["fallback"]
    assert fb_on >= 1 + len(rescued), (fb_on, rescued)          # frame 0 and every frame that needed SLAM()'s second update
    assert fb_off - fb_on >= skips_step - skips_blk >= 1, (fb_off, fb_on, skips_step, skips_blk)      # the un-rescued outlier frames went through blocks
