"""CPU tests of the numpy restatement of on-device feature detection (tests/np_detect.py): the Shi-Tomasi response, GFTT's selection
and the filter pass of detectAndfilteringFeatures (SLAM.cpp:574-768).  The GPU tests hold the device to this restatement bit for bit."""
import numpy as np

import np_detect as D


def squares_image(H=240, W=320, squares=((40, 50, 60), (150, 60, 50), (60, 200, 70), (170, 220, 40))):
    img = np.zeros((H, W), dtype=np.uint8)
    for (y, x, s) in squares:
        img[y:y + s, x:x + s] = 255
    corners = []
    for (y, x, s) in squares:
        corners += [(x, y), (x + s - 1, y), (x, y + s - 1), (x + s - 1, y + s - 1)]
    return img, np.array(corners)


def test_squares_corners_found_within_one_pixel():
    img, corners = squares_image()
    uv, loops = D.detect(img, max_corners=32, quality=0.1, min_dist=10.0, border=5, unfiltered=True)
    assert len(loops) == 0
    assert len(uv) == len(corners)
    for c in corners:
        assert np.abs(uv - c).max(axis=1).min() <= 1, c
    for p in uv:
        assert np.abs(corners - p).max(axis=1).min() <= 1, p


def test_min_distance_and_descending_response():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(120, 160)).astype(np.float64)
    k = np.ones(5) / 5
    img = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), 0, img)
    img = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), 1, img).astype(np.uint8)
    kp = D.gftt(img, max_corners=200, quality=0.01, min_dist=7.0)
    assert len(kp) > 20
    d2 = ((kp[:, None, :] - kp[None, :, :]) ** 2).sum(-1) + np.eye(len(kp), dtype=np.int64) * 10 ** 9
    assert d2.min() >= 49
    r = D.response(img)
    rk = r[kp[:, 1], kp[:, 0]]
    assert np.all(np.diff(rk) <= 0)


def test_ties_go_in_raster_order():
    img = np.zeros((64, 64), dtype=np.uint8)
    for y in range(8, 56, 12):
        for x in range(8, 56, 12):
            img[y:y + 4, x:x + 4] = 200                 # identical blobs: exactly tied responses
    r = D.response(img)
    kp = D.gftt(img, max_corners=0, quality=0.5, min_dist=0.0, cap=10000)
    rk = r[kp[:, 1], kp[:, 0]]
    for a in range(len(kp) - 1):
        if rk[a] == rk[a + 1]:
            assert kp[a, 1] * 64 + kp[a, 0] < kp[a + 1, 1] * 64 + kp[a + 1, 0]
    assert len(set(rk.tolist())) < len(rk)           # there were ties to order


def test_integer_sums_stay_below_2_53():
    assert D.integer_bound(3) < 2 ** 53 and D.integer_bound(5) < 2 ** 53
    assert D.integer_bound(7) >= 2 ** 53              # why other block sizes are refused
    # the extreme frame: a one-pixel checkerboard of 0 / 255 (|Ix|, |Iy| at their maximum where the pattern allows)
    img = ((np.indices((32, 32)).sum(0) % 2) * 255).astype(np.uint8)
    for b in (3, 5):
        gx, gy = D.gradients(img)
        A, B, C = D.box_sum(gx * gx, b), D.box_sum(gx * gy, b), D.box_sum(gy * gy, b)
        assert int(((A + C) ** 2).max()) <= D.integer_bound(b)
        assert np.all((A - C) ** 2 + 4 * B ** 2 <= (A + C) ** 2)


def test_flat_frame_has_no_corners():
    uv, loops = D.detect(np.full((48, 64), 77, dtype=np.uint8), unfiltered=True, border=2)
    assert uv.shape == (0, 2) and loops.shape == (0, 2)


def test_filter_border():
    kps = np.array([[19, 100], [20, 100], [620, 100], [621, 100], [100, 460], [100, 461]])
    uv, _ = D.filter_pass(kps, 640, 480, unfiltered=True)
    assert uv.tolist() == [[20, 100], [620, 100], [100, 460]]


def test_filter_unfiltered_skips_every_other_rule():
    kps = np.array([[100, 100], [101, 100]])
    uv, loops = D.filter_pass(kps, 640, 480, unfiltered=True, map_px=[[100, 100, 100, 100]], map_gate=True, arch_px=[[100, 100]])
    assert len(uv) == 2 and len(loops) == 0


def test_filter_map_veto_and_zero_quirk():
    kps = np.array([[100, 100], [300, 300]])
    mp = [[105, 100, 400, 400]]                          # matched location close to the first key point
    uv, _ = D.filter_pass(kps, 640, 480, map_px=mp, map_gate=True)
    assert uv.tolist() == [[300, 300]]
    uv, _ = D.filter_pass(kps, 640, 480, map_px=mp, map_gate=False)
    assert len(uv) == 2                                  # m_nMatches == 0: no veto
    mp = [[500, 400, 0, 300]]                            # one zero among the four values rejects every key point
    uv, _ = D.filter_pass(kps, 640, 480, map_px=mp, map_gate=True)
    assert len(uv) == 0
    mp = [[100, 114, 500, 400]]                          # 14^2 < 15^2: close; 15^2 is not
    assert len(D.filter_pass(kps[:1], 640, 480, map_px=mp, map_gate=True)[0]) == 0
    mp = [[100, 115, 500, 400]]
    assert len(D.filter_pass(kps[:1], 640, 480, map_px=mp, map_gate=True)[0]) == 1


def test_filter_loop_points_without_break():
    kps = np.array([[100, 100], [200, 200], [300, 300]])
    arch = [[102, 100], [400, 400], [99, 104], [200, 214], [0, 0]]
    uv, loops = D.filter_pass(kps, 640, 480, arch_px=arch)
    assert loops.tolist() == [[0, 0], [0, 2], [1, 3]]
    assert uv.tolist() == [[300, 300]]
    # with a map veto the archive is not consulted for that key point
    uv, loops = D.filter_pass(kps, 640, 480, map_px=[[101, 101, 101, 101]], map_gate=True, arch_px=arch)
    assert loops.tolist() == [[1, 3]]


def test_filter_pairwise():
    kps = np.array([[100, 100], [110, 100], [116, 100], [100, 120]])
    uv, _ = D.filter_pass(kps, 640, 480)
    assert uv.tolist() == [[100, 100], [116, 100], [100, 120]]


def test_schedule_repeats_until_enough_or_above_30():
    img, _ = squares_image()
    # steady state (frame 5), map of 1, key points sparse: the loop runs while the running count is below m_minNUM, at most until
    # m_nInitialRaws (8 -> 13 -> 18 -> 23 -> 28 -> 33) passes 30; m_nProcessRaws stays the corner budget
    passes = D.add_features_schedule(img, frame_counter=5, is_adding=False, first_call=False, n_map=1, n_matches=0, map_px=None,
                                     arch_px=None, n_process=1, border=5)
    assert [p["max_corners"] for p in passes] == [1] * len(passes)
    assert passes[-1]["running"] >= 5 or len(passes) == 5
    assert all(len(p["uv"]) == 1 for p in passes)
    assert [p["running"] for p in passes] == [2, 3, 4, 5]
    # frame 1: m_nInitialRaws grows with the passes
    passes = D.add_features_schedule(np.zeros((240, 320), np.uint8), frame_counter=1, is_adding=False, first_call=True, n_map=0,
                                     n_matches=0, map_px=None, arch_px=None)
    assert [p["max_corners"] for p in passes] == [8, 13, 18, 23, 28]
    assert all(p["unfiltered"] for p in passes)
