"""GPU tests of the colour-frame intake and the 2-D feature overlay (srukf_set_frame_bgr / srukf_associate_held / srukf_render_overlay, include/srukf.h;
csrc/srukf_overlay.hip): every byte must EQUAL the numpy restatement (tests/np_overlay.py); the held frame must be what srukf_associate would have uploaded; the
calls must leave the filter's results untouched on both step paths; the colour frame must follow the handle through map changes; and the CSLAM facade's host
(host/cslam_vision.cpp colour=1 / overlay=<file>) must give the default run's trajectory and the restatement's overlay."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_overlay as OV
from test_gpu_detect import VISION, _run_vision, params, squares, texture

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


def colour_frame(seed, H, W):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def random_landmarks(seed, N, W, H):
    """centres inside and up to 20 px outside the frame, Si of every orientation with semi-axes from 1 to ~60 px, four in five matched"""
    rng = np.random.default_rng(seed)
    h = np.stack([rng.uniform(-20, W + 20, N), rng.uniform(-20, H + 20, N)], axis=1)
    z = h + rng.normal(0.0, 6.0, (N, 2))
    Si = rng.normal(0.0, 1.0, (N, 4)) * (10.0 ** rng.uniform(-1.0, 1.3, (N, 1)))
    Si[::3, 2] = 0.0                                             # (upper triangular, as the filter's)
    m = (rng.uniform(size=N) < 0.8).astype(np.int32)
    m[0] = 1
    return h, Si, z, m


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("W,H", [(640, 480), (70, 50)])
@pytest.mark.parametrize("N", [1, 3, 65, 130])
def test_overlay_equals_the_restatement(srukf, synth, W, H, N):
    """640 x 480, and 70 x 50: no multiple of the 1024-pixel tile, rows that are no multiple of four pixels (groups straddle rows).  N = 65 and 130 exceed one
    wave and one 64-landmark chunk."""
    f = srukf.Filter(N, params(synth, W, H))
    bgr = colour_frame(100 + N, H, W)
    f.set_frame_bgr(bgr, want_gray=False)
    h, Si, z, m = random_landmarks(N, N, W, H)
    out = f.render_overlay(h, Si, z, m)
    ref = OV.render(bgr, h, Si, z, m)
    assert (ref != bgr).any()
    assert np.array_equal(out, ref), np.argwhere((out != ref).any(axis=2))[:10]
    f.close()


@pytest.mark.parametrize("W,H", [(640, 480), (70, 50), (71, 51), (9, 9)])
def test_gray_conversion_exact(srukf, synth, W, H):
    """71 x 51 and 9 x 9: W H = 1 (mod 4), the frame ends in a group of one pixel (byte-wide tail); 70 x 50: whole groups that straddle rows"""
    f = srukf.Filter(0, params(synth, W, H))
    for seed in (1, 2):
        bgr = colour_frame(seed, H, W)
        g = f.set_frame_bgr(bgr)
        assert np.array_equal(g, OV.gray(bgr))
    v = np.random.default_rng(3).integers(0, 256, size=(H, W), dtype=np.uint8)
    assert np.array_equal(f.set_frame_bgr(np.stack([v, v, v], axis=-1)), v)       # a gray frame is kept byte for byte
    # ... and the overlay of the held pair on the same odd sizes, colour and gray source
    out = f.render_overlay(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int32))
    assert np.array_equal(out, np.stack([v, v, v], axis=-1))
    f.close()


SYM_UV = np.array([[100.0, 90.0], [220.0, 150.0], [340.0, 80.0], [470.0, 200.0], [560.0, 330.0], [150.0, 300.0], [300.0, 390.0], [420.0, 300.0]])


def symmetric_blobs(seed):
    """A textured 640 x 480 frame with a 45 x 45 block B = B^T centred on each of SYM_UV.  wrapPatch writes the template with its x index as the row (SLAM.cpp:1899,
    kept by k_warp_patch), so the reference's correlation compares the frame with the TRANSPOSED patch: only a patch that equals its transpose can exceed the 0.8
    of THRESHOLD_MATCH_PATCH.  These do."""
    img = texture(seed).copy()
    rng = np.random.default_rng(seed)
    for u, v in SYM_UV.astype(int):
        R = rng.integers(0, 256, size=(49, 49)).astype(np.float64)
        c = np.cumsum(np.cumsum(R, 0), 1)
        R = (c[4:, 4:] - c[:-4, 4:] - c[4:, :-4] + c[:-4, :-4]) / 16.0          # 4 x 4 box mean, 45 x 45
        img[v - 22:v + 23, u - 22:u + 23] = (0.5 * (R + R.T)).astype(np.uint8)
    return img


def test_associate_held_sees_gray_out(srukf, synth):
    """gray_out is the held frame: associating on it through srukf_associate(gray_out) and through srukf_set_frame_bgr + srukf_associate_held gives equal z,
    matched and corr (the appearance records come from srukf_capture_appearance(gray = NULL) on both filters)."""
    p = params(synth)
    img = symmetric_blobs(21)
    rng = np.random.default_rng(5)
    bgr2 = np.clip(img.astype(np.int16)[:, :, None] + rng.integers(-3, 4, size=(480, 640, 3)), 0, 255).astype(np.uint8)      # a colour frame whose gray is near img
    S4 = np.diag([p["sigma_x"], p["sigma_y"], p["sigma_z"], p["sigma_theta"]])
    X4 = np.array([0.1, 0.05, 0.0, 0.0])
    A, B = srukf.Filter(0, p), srukf.Filter(0, p)
    for f in (A, B):
        f.set_state(X4, S4)
        f.detect_features(img, max_corners=10, unfiltered=True)  # (brings the frame)
        f.add_landmarks(SYM_UV)
        f.capture_appearance(0, SYM_UV)                          # the held frame (it survived add_landmarks)
        with pytest.raises(srukf.SrukfError) as e:
            f.associate_held()                                   # before predict_measurement
        assert e.value.rc == -5
        f.predict_motion(np.zeros(3), np.zeros(3))              # the pose of the capture: the warp is the identity view (the oracle's restatement gives
        f.predict_measurement()                                  # corr 0.99 for all eight blobs here, and below 0.65 once a freshly initialised map has moved 1 cm)
    gray2 = B.set_frame_bgr(bgr2)
    assert np.array_equal(gray2, OV.gray(bgr2)) and (gray2 != img).any()
    rb = B.associate_held()
    ra = A.associate(gray2)
    print("matched", ra[1], "corr", np.round(ra[2], 3))
    assert same_bits(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and same_bits(ra[2], rb[2])
    assert ra[1].sum() >= 3 and np.abs(ra[2]).max() > 0.8        # landmarks did match
    assert all(np.array_equal(A.get_match_patch(k), B.get_match_patch(k)) for k in range(A.N))
    A.close(); B.close()


CRAFTED = [
    # h, Si (row-major s00 s01 s10 s11), z, matched
    ((30.0, 30.0), (3.0, 0.0, 0.0, 3.0), (34.0, 31.0), 0),                  # unmatched: not drawn
    ((20.0, 100.0), (0.0, 0.0, 0.0, 0.0), (24.0, 104.0), 1),               # Si = 0: a = b = 1
    ((60.0, 30.0), (2.0, 0.0, 0.0, 6.0), (62.0, 33.0), 1),                 # p01 = 0, d < 0: upright
    ((100.0, 30.0), (3.0, 1.0, 1.0, 3.0), (101.0, 32.0), 1),               # d = 0, p01 != 0: 45 degrees
    ((130.0, 70.0), (2.0, 3.0, 0.0, 5.0), (128.0, 72.0), 1),               # d < 0, p01 != 0
    ((40.0, 70.0), (NAN, 0.0, 0.0, 2.0), (45.0, 74.0), 1),                 # NaN in Si: crosses, no ellipse
    ((70.0, 100.0), (1e6, 0.0, 0.0, 1.0), (74.0, 98.0), 1),                # l0 = 1e12: no ellipse
    ((0.0, 0.0), (4.0, 1.0, 0.0, 2.0), (159.0, 119.0), 1),                 # centres on the image border
    ((-5.0, 60.0), (8.0, 0.0, 0.0, 3.0), (170.0, -8.0), 1),                # ... and outside it, reaching in
    ((-400.0, 60.0), (2.0, 0.0, 0.0, 2.0), (1000.0, 1000.0), 1),           # ... and out of reach
    ((80.0, 60.0), (100.0, 0.0, 0.0, 90.0), (80.0, 60.0), 1),              # an ellipse larger than the image: the band lies outside
    ((85.0, 55.0), (30.0, 5.0, 0.0, 20.0), (82.0, 58.0), 1),               # ... and one that is cut by all four borders
    ((NAN, 5.0), (2.0, 0.0, 0.0, 2.0), (50.0, 50.0), 1),                   # h not finite: skipped
    ((50.0, 50.0), (2.0, 0.0, 0.0, 2.0), (50.0, INF), 1),                  # z not finite: skipped
    ((2.0 ** 30, 50.0), (2.0, 0.0, 0.0, 2.0), (50.0, 50.0), 1),            # 2^30: skipped
    ((2.0 ** 30 - 1, 50.0), (2.0, 0.0, 0.0, 2.0), (-2.0 ** 30 + 1, 50.0), 1),     # just below: drawn, out of reach
    ((30.5, 41.5), (1.5, 0.0, 0.0, 1.0), (110.5, 99.5), 1),                # half-integer centres: ties to even (30, 42), (110, 100)
    ((140.0, 20.0), (1e-160, 0.0, 1e-170, 2e-160), (143.0, 22.0), 1),      # squares at the bottom of the exponent range
]


def _arrays(rows):
    h = np.array([r[0] for r in rows]); Si = np.array([r[1] for r in rows]); z = np.array([r[2] for r in rows])
    return h, Si, z, np.array([r[3] for r in rows], dtype=np.int32)


def test_crafted_landmarks(srukf, synth):
    W, H = 160, 120
    bgr = colour_frame(7, H, W)
    f = srukf.Filter(len(CRAFTED), params(synth, W, H))
    f.set_frame_bgr(bgr, want_gray=False)
    h, Si, z, m = _arrays(CRAFTED)
    out = f.render_overlay(h, Si, z, m)
    ref = OV.render(bgr, h, Si, z, m)
    assert np.array_equal(out, ref), np.argwhere((out != ref).any(axis=2))[:10]
    recs = OV.prep(h, Si, z, m)
    assert [r["drawn"] for r in recs] == [False] + [True] * 11 + [False] * 3 + [True] * 3
    assert [r["ellipse"] for r in recs[1:12]] == [True, True, True, True, False, False, True, True, True, True, True]
    assert (recs[1]["a"], recs[1]["b"]) == (1, 1) and (recs[16]["px"], recs[16]["py"], recs[16]["mx"], recs[16]["my"]) == (30, 42, 110, 100)
    assert tuple(out[0, 0]) == OV.BLUE and tuple(out[119, 159]) == OV.RED
    f.close()
    # each landmark alone (its own boxes decide which tiles list it)
    g = srukf.Filter(1, params(synth, W, H))
    g.set_frame_bgr(bgr, want_gray=False)
    for row in CRAFTED:
        a = _arrays([row])
        assert np.array_equal(g.render_overlay(*a), OV.render(bgr, *a)), row
    g.close()


def test_paint_order_later_over_earlier(srukf, synth):
    W, H = 160, 120
    bgr = colour_frame(8, H, W)
    f = srukf.Filter(2, params(synth, W, H))
    f.set_frame_bgr(bgr, want_gray=False)
    one = ((80.0, 60.0), (4.0, 0.0, 0.0, 2.0), (20.0, 20.0), 1)             # predicted (blue) cross at (80, 60)
    two = ((30.0, 100.0), (4.0, 2.0, 0.0, 3.0), (80.0, 60.0), 1)           # matched (red) cross and ellipse at (80, 60)
    outs = []
    for rows in ([one, two], [two, one]):
        a = _arrays(rows)
        out = f.render_overlay(*a)
        assert np.array_equal(out, OV.render(bgr, *a))
        outs.append(out)
    assert tuple(outs[0][60, 80]) == OV.RED and tuple(outs[1][60, 80]) == OV.BLUE
    assert (outs[0] != outs[1]).any()
    f.close()


def test_source_selection_and_errors(srukf, synth):
    p = params(synth)
    N = 8
    sc = synth.make_scene(N, 2, seed=3, p=p)
    f = srukf.Filter(N, p); f.set_state(sc["X0"], sc["S0"])
    zero = (np.zeros(2 * N), np.zeros(4 * N), np.zeros(2 * N), np.zeros(N, dtype=np.int32))
    lm = random_landmarks(4, N, 640, 480)
    for call in (lambda: f.render_overlay(*zero), f.associate_held):
        with pytest.raises(srukf.SrukfError) as e:
            call()                                               # no frame held
        assert e.value.rc == -5
    lib, hd, ub = f._lib, f._h, C.POINTER(C.c_ubyte)
    bgr, gray = colour_frame(9, 480, 640), texture(9)
    buf = np.zeros((480, 640, 3), dtype=np.uint8)
    assert lib.srukf_set_frame_bgr(hd, None, None) == -1 and lib.srukf_set_frame_bgr(None, bgr.ctypes.data_as(ub), None) == -1
    f.set_frame_bgr(bgr)
    assert lib.srukf_render_overlay(hd, None, None, None, None, buf.ctypes.data_as(ub)) == -1
    assert lib.srukf_render_overlay(hd, zero[0].ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None) == -1
    assert lib.srukf_associate_held(None, None, None, None) == -1
    assert np.array_equal(f.render_overlay(*zero), bgr)          # nothing matched: the colour frame itself
    assert np.array_equal(f.render_overlay(*lm), OV.render(bgr, *lm))
    with pytest.raises(srukf.SrukfError) as e:
        f.associate_held()                                       # a frame is held, but before predict_measurement
    assert e.value.rc == -5
    # a gray frame passed later replaces the gray one and invalidates the colour one
    f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement()
    f.associate(gray)
    assert np.array_equal(f.render_overlay(*zero), np.repeat(gray[:, :, None], 3, axis=2))
    assert np.array_equal(f.render_overlay(*lm), OV.render(gray, *lm))
    f.set_frame_bgr(bgr)
    assert np.array_equal(f.render_overlay(*zero), bgr)
    f.detect_features(gray, unfiltered=True)
    assert np.array_equal(f.render_overlay(*zero), np.repeat(gray[:, :, None], 3, axis=2))
    f.set_frame_bgr(bgr)
    f.detect_features(None, unfiltered=True)                     # the held gray frame: the colour one stays
    assert np.array_equal(f.render_overlay(*zero), bgr)
    f.update(sc["z"][0], sc["matched"][0])
    assert np.array_equal(f.render_overlay(*lm), OV.render(bgr, *lm))       # valid in any phase
    f.close()


@pytest.mark.parametrize("path", ["fast_next", "slow"])
def test_calls_leave_the_filter_untouched(srukf, synth, path):
    """Twin filters, fp64 storage, fed the same z: one calls set_frame_bgr, associate_held and render_overlay between predict_measurement and update (and the
    overlay once more behind the update, where the next frame's first launch may be in flight).  X and S stay bit-identical."""
    p = params(synth)
    N, F = 60, 5
    sc = synth.make_scene(N, 10, seed=31, p=p)
    a, b = srukf.Filter(N, p), srukf.Filter(N, p)
    for f in (a, b):
        f.set_state(sc["X0"], sc["S0"])
        if path == "slow":
            f.debug_set("step_fast", 0)
    bgr = colour_frame(11, 480, 640)
    for t in range(F):
        outs = []
        for f in (a, b):
            f.predict_motion(sc["odo"][t], sc["odo"][t + 1])
            if path == "fast_next":
                f.predict_motion_next(sc["odo"][t + 1], sc["odo"][t + 2])
            h, Si, vis = f.predict_measurement()
            if f is a:
                a.set_frame_bgr(bgr)
                a.associate_held()
                z, m = sc["z"][t], sc["matched"][t]
                out = a.render_overlay(h, Si, z, m)
                if t == F - 1:
                    assert np.array_equal(out, OV.render(bgr, h, Si, z, m)) and (out != bgr).any()
            f.update(sc["z"][t], sc["matched"][t])
            if f is a:
                a.render_overlay(h, Si, sc["z"][t], sc["matched"][t])
        Xa, Sa = a.get_state(); Xb, Sb = b.get_state()
        assert same_bits(Xa, Xb) and same_bits(Sa, Sb), t
    nf = (a.debug_get("step_fast"), b.debug_get("step_fast"))
    assert nf == ((F - 1, F - 1) if path == "fast_next" else (0, 0)), nf
    prof_names = a.profile().keys()
    assert "k_bgr2gray" in prof_names and "k_overlay" in prof_names
    a.close(); b.close()


def test_colour_frame_follows_the_handle_through_map_changes(srukf, synth):
    p = params(synth)
    N = 8
    sc = synth.make_scene(N, 2, seed=3, p=p)
    f = srukf.Filter(N, p); f.set_state(sc["X0"], sc["S0"])
    bgr = colour_frame(12, 480, 640)
    f.set_frame_bgr(bgr)

    def check():
        lm = random_landmarks(20 + f.N, f.N, 640, 480)
        assert np.array_equal(f.render_overlay(*lm), OV.render(bgr, *lm))

    check()
    f.delete_landmark(3); assert f.N == N - 1                    # a new context
    check()
    f.add_landmarks(np.array([[300.0, 200.0]])); assert f.N == N         # the retired context of N = 8, revived: it supplies no frame of its own
    check()
    f.add_landmarks(np.array([[340.0, 260.0], [200.0, 300.0]])); assert f.N == N + 2
    check()
    f.delete_landmark(0); f.delete_landmark(0); assert f.N == N          # revived once more
    check()
    f.reset()
    with pytest.raises(srukf.SrukfError) as e:
        f.render_overlay(np.zeros(2 * N), np.zeros(4 * N), np.zeros(2 * N), np.zeros(N, dtype=np.int32))
    assert e.value.rc == -5                                      # srukf_reset drops the held frames
    f.set_frame_bgr(bgr)
    check()
    f.close()


def _read_rows(path):
    rows = [[float.fromhex(v) for v in l.split()[:8]] + [int(l.split()[8])] for l in open(path) if l.strip()]
    a = np.array(rows, dtype=np.float64).reshape(-1, 9)
    return a[:, 0:2], a[:, 2:6], a[:, 6:8], a[:, 8].astype(np.int32)


def test_host_colour_intake_and_overlay(tmp_path, synth):
    """cslam_vision colour=1 (every frame through loadPictures + dataAssociationOnDeviceHeld as a B = G = R colour frame) prints the default run's trajectory, and
    overlay=<file> holds the restatement applied to the rows in <file>.in and the last frame, on both runs."""
    assert os.path.exists(VISION), "run __graft_entry__.build() first"
    # a static scene and a robot at rest: every frame is the identity view of the landmarks' creation, where the reference's warped patches do match (a freshly
    # initialised map that has moved correlates below 0.8: the oracle's restatement says so too), so the overlay has something to draw
    frames = [squares()] * 4
    odo = [(0.0, 0.0, 0.0)] * 6
    outs = []
    for mode in ("default", "colour"):
        d = tmp_path / mode
        d.mkdir()
        extra = [f"overlay={d}/ov.bin"] + (["colour=1"] if mode == "colour" else [])
        out = _run_vision(str(d), frames, odo, *extra)
        lines = [l for l in out.splitlines() if not l.startswith("add_features_frame1_ms")]
        assert sum(l.startswith("pose ") for l in lines) == 5
        ov = np.fromfile(f"{d}/ov.bin", dtype=np.uint8).reshape(480, 640, 3)
        h, Si, z, m = _read_rows(f"{d}/ov.bin.in")
        assert len(m) >= 5 and m.sum() >= 1
        ref = OV.render(frames[(5 - 1) % 4], h, Si, z, m)
        assert np.array_equal(ov, ref) and (ov != np.repeat(frames[0][:, :, None], 3, axis=2)).any()
        outs.append((lines, ov))
    assert outs[0][0] == outs[1][0]
    assert np.array_equal(outs[0][1], outs[1][1])
