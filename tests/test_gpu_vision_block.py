"""GPU test of the block-wise facade (CSLAM::SLAMBlock through cslam_vision block=<F>): the same synthetic sequence through block=8 and through
block=1 (the step-wise route, SLAM() per frame, with the same report lines).

Sequence: tests/test_gpu_images.py's smooth texture (seed 17) rolled one pixel per frame under a robot that moves 1 cm per frame, 24 frames, 640 x 480; the map is
what the facade's own detection finds in frame 0 (8 corners, of which 4 match from frame to frame: min_matches=4, since with m_minNUM = 5 every frame of this
sequence asks for an addition and no block could run on).  Landmarks leave through updateFeaturesInformation around frames 10 and 21, and addFeatures finds new
ones behind them.  The sequence was chosen from runs of the step-wise route on the device (12 candidates: 4 textures, 3 roll speeds), not with the oracle's
association on the CPU, so the correlation margins of DESIGN.md §20 and the 1e-6 distance of the policy's real-valued tests from their thresholds are NOT
vetted for it.  Asserted on the block=1 run alone, before any comparison: at least one deletion and at least one addition behind frame 0.  Compared: the deleted IDs of every frame, the additions of every frame, the map's IDs behind every frame,
and every path row within the project's per-frame bounds (|dX| <= 1e-9, |dP| <= 1e-11); at least one block stopped early and at least one ran all 8 frames."""
import os

import numpy as np
import pytest

import test_gpu_detect as TD
from test_gpu_unique import _texture

pytestmark = pytest.mark.gpu

TOL_X, TOL_P = 1e-9, 1e-11
FRAMES, ROLL, BLOCK, MIN_MATCHES = 24, 1, 8, 4


def _rows(out, key):
    return [ln.split()[1:] for ln in out.splitlines() if ln.split() and ln.split()[0] == key]


def _report(out):
    pol = _rows(out, "policy")
    frames = [int(r[1]) for r in pol]
    deleted = [[int(v) for v in r[4:4 + int(r[3])]] for r in pol]
    added = [int(r[-1]) for r in pol]
    ids = {int(f[0]): [int(v) for v in i] for f, i in zip(_rows(out, "frame"), _rows(out, "ids"))}
    path = {int(p[0]): np.array([float(v) for v in p[1:]]) for p in _rows(out, "path")}
    t = _rows(out, "blocks")[0]                                  # "blocks <n> early <n> full <n> fallback <n>" without its first word
    return dict(frames=frames, deleted=deleted, added=added, ids=ids, path=path, blocks={"blocks": int(t[0]), t[1]: int(t[2]), t[3]: int(t[4]), t[5]: int(t[6])})


def test_block_route_equals_the_stepwise_route(tmp_path):
    assert os.path.exists(TD.VISION), "run __graft_entry__.build() first"
    base = _texture(np.random.default_rng(17))
    frames = [np.roll(base, (0, ROLL * q), axis=(0, 1)) for q in range(FRAMES)]
    odo = [(0.01 * i, 0.0, 0.0) for i in range(FRAMES + 1)]
    d1, d8 = tmp_path / "step", tmp_path / "block"
    d1.mkdir(); d8.mkdir()
    out1 = TD._run_vision(str(d1), frames, odo, "block=1", f"min_matches={MIN_MATCHES}")
    step = _report(out1)
    out8 = TD._run_vision(str(d8), frames, odo, f"block={BLOCK}", f"min_matches={MIN_MATCHES}")
    blk = _report(out8)
    print("step-wise: deleted", step["deleted"], "added", step["added"])
    print("block-wise:", blk["blocks"], [ln for ln in (out1 + out8).splitlines() if ln.startswith("block_frames")])
    # the sequence does what it was chosen for (the reference run alone)
    assert step["frames"] == list(range(FRAMES))
    assert sum(len(d) for d in step["deleted"]) >= 1 and sum(step["added"][1:]) >= 1
    # the comparison
    assert blk["frames"] == step["frames"]
    assert blk["deleted"] == step["deleted"]
    assert blk["added"] == step["added"]
    assert sorted(blk["ids"]) and all(blk["ids"][f] == step["ids"][f] for f in blk["ids"])
    assert blk["ids"][FRAMES - 1] == step["ids"][FRAMES - 1]
    dx = max(np.abs(blk["path"][f][:4] - step["path"][f][:4]).max() for f in blk["path"])
    dp = max(np.abs(blk["path"][f][4:] - step["path"][f][4:]).max() for f in blk["path"])
    print("path rows compared: %d, |dX| %.3e, |dP| %.3e" % (len(blk["path"]), dx, dp))
    assert dx <= TOL_X and dp <= TOL_P
    assert sorted(blk["path"]) == list(range(FRAMES)) == sorted(step["path"])
    assert blk["blocks"]["early"] >= 1 and blk["blocks"]["full"] >= 1, blk["blocks"]
