"""GPU test of the display view through the block-wise facade (CSLAM::blockDisplay / m_blockDisplay / renderBlockOverlay through cslam_vision block=<F>
display=<file>): tests/test_gpu_vision_block.py's 24-frame sequence through block=8 and through block=1, each writing the display view of every
landmark of the map behind every frame (frame, ID, xyz, cov, axis, sigma as %a; a NaN as "nan").  The last consumed frame of a block is written from map[] behind
SLAM()'s own tail, as every frame of block=1 is; the frames in front of it from the record the block's frames left on the device.

Required: the two files are identical as text, and the path, frame, ids and policy lines on stdout are what they are without display=.  The same with resume=1.
The largest numeric difference between the two files is printed before the comparison."""
import os

import numpy as np
import pytest

import test_gpu_detect as TD
from test_gpu_unique import _texture
from test_gpu_vision_block import BLOCK, FRAMES, MIN_MATCHES, ROLL

pytestmark = pytest.mark.gpu

KEEP = ("path", "frame", "ids", "policy")


def _kept(out):
    return [ln for ln in out.splitlines() if ln.split() and ln.split()[0] in KEEP]


def _numbers(text):
    rows = {}
    for ln in text.splitlines():
        t = ln.split()
        rows[(int(t[0]), int(t[1]))] = np.array([float("nan") if v == "nan" else float.fromhex(v) for v in t[2:]])
    return rows


@pytest.mark.parametrize("resume", [0, 1])
def test_block_route_writes_the_stepwise_routes_display(tmp_path, resume):
    assert os.path.exists(TD.VISION), "run __graft_entry__.build() first"
    base = _texture(np.random.default_rng(17))
    frames = [np.roll(base, (0, ROLL * q), axis=(0, 1)) for q in range(FRAMES)]
    odo = [(0.01 * i, 0.0, 0.0) for i in range(FRAMES + 1)]
    extra = [f"min_matches={MIN_MATCHES}"] + (["resume=1"] if resume else [])
    dirs = {}
    for name in ("step", "block", "step_plain", "block_plain"):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
    fa, fb, fo = str(dirs["block"] / "display.txt"), str(dirs["step"] / "display.txt"), str(dirs["block"] / "overlay.bgr")
    out8 = TD._run_vision(str(dirs["block"]), frames, odo, f"block={BLOCK}", f"display={fa}", f"overlay={fo}", *extra)
    out1 = TD._run_vision(str(dirs["step"]), frames, odo, "block=1", f"display={fb}", *extra)
    plain8 = TD._run_vision(str(dirs["block_plain"]), frames, odo, f"block={BLOCK}", *extra)
    plain1 = TD._run_vision(str(dirs["step_plain"]), frames, odo, "block=1", *extra)
    # stdout is what it is without display=
    assert _kept(out8) == _kept(plain8) and _kept(out1) == _kept(plain1)
    blocks = [ln for ln in out8.splitlines() if ln.startswith("blocks")][0].split()
    assert int(blocks[1]) >= 2 and int(blocks[5]) >= 1, blocks     # frames in front of a block's last one exist: some lines come from the record
    A, B = open(fa).read(), open(fb).read()
    a, b = _numbers(A), _numbers(B)
    assert len(a) > FRAMES and sorted(a) == sorted(b)             # the same frames and IDs, line by line
    assert sorted({k[0] for k in a}) == list(range(FRAMES))
    d = max((np.abs(a[k] - b[k])[~(np.isnan(a[k]) & np.isnan(b[k]))].max(initial=0.0) for k in a))
    differ = sum(1 for la, lb in zip(A.splitlines(), B.splitlines()) if la != lb)
    print("display lines %d, lines that differ %d, largest |difference| %.3e (resume=%d)" % (len(a), differ, d, resume))
    # the overlay of the last block's last consumed frame: the frame with something drawn on it
    img = np.fromfile(fo, dtype=np.uint8)
    assert img.size == 640 * 480 * 3
    drawn = min(int((img != np.repeat(fr[:, :, None], 3, axis=2).reshape(-1)).sum()) for fr in frames)
    print("overlay bytes that differ from the nearest bare frame: %d" % drawn)
    assert 0 < drawn < img.size // 20                            # one of the sequence's frames, with crosses and ellipses on it
    assert A == B
