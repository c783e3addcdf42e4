"""GPU test of CSLAM::deleteTogether through cslam_vision together=1: tests/test_gpu_vision_block.py's 24-frame sequence through the step-wise
route without the option (the reference run), with it, and with it through block=8.

Asserted on the reference run alone, from its printed lines: a frame deletes at least two landmarks, and a landmark right behind a deleted one in the state
leaves one frame later (the walk of updateFeaturesInformation does not test the node that slides into a deleted position; both neighbours tested positive, the
second was skipped).  Compared with the reference run, for both runs with the option: the deleted IDs of every frame, the additions of every frame, the map's IDs
behind every frame, and every path row within the project's per-frame bounds (|dX| <= 1e-9, |dP| <= 1e-11)."""
import os

import numpy as np
import pytest

import test_gpu_detect as TD
from test_gpu_unique import _texture
from test_gpu_vision_block import BLOCK, FRAMES, MIN_MATCHES, ROLL, TOL_P, TOL_X, _report

pytestmark = pytest.mark.gpu


def test_together_equals_one_by_one_stepwise_and_blockwise(tmp_path):
    assert os.path.exists(TD.VISION), "run __graft_entry__.build() first"
    base = _texture(np.random.default_rng(17))
    frames = [np.roll(base, (0, ROLL * q), axis=(0, 1)) for q in range(FRAMES)]
    odo = [(0.01 * i, 0.0, 0.0) for i in range(FRAMES + 1)]
    runs = {}
    for name, args in (("one_by_one", ["block=1"]), ("together", ["block=1", "together=1"]), ("together_block", [f"block={BLOCK}", "together=1"])):
        d = tmp_path / name
        d.mkdir()
        runs[name] = _report(TD._run_vision(str(d), frames, odo, *args, f"min_matches={MIN_MATCHES}"))
    ref = runs["one_by_one"]
    print("one by one: deleted", [(f, d) for f, d in enumerate(ref["deleted"]) if d], "added", [(f, a) for f, a in enumerate(ref["added"]) if a])
    # the sequence holds what the option is for (the reference run alone)
    assert ref["frames"] == list(range(FRAMES))
    many = [f for f, d in enumerate(ref["deleted"]) if len(d) >= 2]
    assert many, "no frame deletes two landmarks"
    skipped = []
    for f in range(1, FRAMES - 1):
        before = ref["ids"][f - 1]
        for a in ref["deleted"][f]:
            at = before.index(a)
            if at + 1 < len(before) and before[at + 1] in ref["deleted"][f + 1] and before[at + 1] not in ref["deleted"][f]:
                skipped.append((f, a, before[at + 1]))
    print("frames that delete several:", many, "neighbours (frame, deleted, the one behind it that leaves a frame later):", skipped)
    assert skipped, "no landmark behind a deleted one leaves a frame later"
    assert sum(ref["added"][1:]) >= 1
    # the comparison
    for name in ("together", "together_block"):
        run = runs[name]
        assert run["frames"] == ref["frames"], name
        assert run["deleted"] == ref["deleted"], name
        assert run["added"] == ref["added"], name
        assert sorted(run["ids"]) and all(run["ids"][f] == ref["ids"][f] for f in run["ids"]), name          # (a block prints the map behind its last frame)
        assert run["ids"][FRAMES - 1] == ref["ids"][FRAMES - 1], name
        if name == "together":
            assert sorted(run["ids"]) == sorted(ref["ids"]) == list(range(FRAMES))
        assert sorted(run["path"]) == list(range(FRAMES)) == sorted(ref["path"]), name
        dx = max(np.abs(run["path"][f][:4] - ref["path"][f][:4]).max() for f in ref["path"])
        dp = max(np.abs(run["path"][f][4:] - ref["path"][f][4:]).max() for f in ref["path"])
        print("%s: path rows compared: %d, |dX| %.3e, |dP| %.3e, blocks %s" % (name, len(ref["path"]), dx, dp, run["blocks"]))
        assert dx <= TOL_X and dp <= TOL_P, name
    assert runs["together_block"]["blocks"]["blocks"] >= 1
