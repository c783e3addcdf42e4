"""GPU tests of feature detection and appearance capture on the device (srukf_detect_features / srukf_capture_appearance, include/srukf.h):
the key points, their order and the loop points must EQUAL the numpy restatement (tests/np_detect.py); a landmark whose appearance was
captured on the device must associate bit for bit like one whose patch the host cut; the CSLAM facade's on-device addFeatures must run
the reference's pass schedule (host/cslam_vision.cpp)."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import np_detect as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VISION = os.path.join(ROOT, "cv-monoslam_amd", "cslam_vision.bin")


def texture(seed, H=480, W=640, k=7):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(H + 2 * k, W + 2 * k)).astype(np.float64)
    c = np.cumsum(np.cumsum(img, 0), 1)
    box = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]
    return (box[:H, :W] / (k * k)).astype(np.uint8)


def squares(H=480, W=640):
    img = np.zeros((H, W), dtype=np.uint8)
    for (y, x, s) in ((60, 80, 90), (250, 100, 120), (100, 350, 70), (300, 420, 100)):
        img[y:y + s, x:x + s] = 255
    return img


def params(synth, W=640, H=480):
    p = dict(synth.scene_params())
    p["image_w"], p["image_h"] = float(W), float(H)
    return p


def check_exact(f, img, **kw):
    uv, loops = f.detect_features(img, **kw)
    ref_kw = dict(max_corners=kw.get("max_corners", 8), quality=kw.get("quality", 0.1), min_dist=kw.get("min_dist", 15.0),
                  block=kw.get("block_size", 3), border=kw.get("border", 20), unfiltered=kw.get("unfiltered", False),
                  map_px=kw.get("map_px"), map_gate=kw.get("map_gate", False), arch_px=kw.get("arch_px"))
    H, W = img.shape
    ruv, rloops = D.detect(img, cap=W * H, **ref_kw)
    assert uv.shape == ruv.shape and np.array_equal(uv, ruv), (uv[:10], ruv[:10])
    assert np.array_equal(loops, rloops), (loops, rloops)
    r = f.debug_copy("det_resp", W * H).reshape(H, W)
    assert np.array_equal(r, D.response(img, ref_kw["block"]))          # the response map itself, bit for bit
    return uv, loops


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_textures_exact(synth, pkg, seed):
    f = pkg.srukf.Filter(0, params(synth))
    img = texture(seed)
    uv, _ = check_exact(f, img, unfiltered=True)
    assert 5 <= len(uv) <= 8                            # (the border drops GFTT corners near the edge)


def test_many_candidates_exact(synth, pkg):
    f = pkg.srukf.Filter(0, params(synth))
    img = texture(7, k=3)
    H, W = img.shape
    assert len(D.candidates(D.response(img), 0.01)) > 2000
    uv, _ = check_exact(f, img, max_corners=500, quality=0.01, min_dist=5.0, unfiltered=True)
    assert len(uv) > 300


def test_squares_exact(synth, pkg):
    f = pkg.srukf.Filter(0, params(synth))
    uv, _ = check_exact(f, squares(), max_corners=32, min_dist=10.0, unfiltered=True)
    assert len(uv) == 16


def test_tied_responses_raster_order(synth, pkg):
    f = pkg.srukf.Filter(0, params(synth))
    img = np.zeros((480, 640), dtype=np.uint8)
    img[::16, :] = 255
    img[:, ::16] = 255                                  # a periodic grid: many exactly tied responses
    uv, _ = check_exact(f, img, max_corners=0, quality=0.5, min_dist=0.0, border=0, unfiltered=True)
    r = D.response(img)
    rk = r[uv[:, 1].astype(int), uv[:, 0].astype(int)]
    assert len(uv) > 100 and (np.diff(rk) == 0).sum() > 50


def test_flat_frame_no_points(synth, pkg):
    f = pkg.srukf.Filter(0, params(synth))
    uv, loops = f.detect_features(np.full((480, 640), 90, dtype=np.uint8), unfiltered=True)
    assert uv.shape == (0, 2) and loops.shape == (0, 2)


def test_small_context(synth, pkg):
    f = pkg.srukf.Filter(0, params(synth, 64, 48))
    img = texture(4, 48, 64, k=3)
    check_exact(f, img, max_corners=20, min_dist=4.0, border=3, unfiltered=True)


def test_block_size_5_and_7(synth, pkg):
    f = pkg.srukf.Filter(0, params(synth))
    img = texture(5)
    check_exact(f, img, max_corners=40, block_size=5, unfiltered=True)
    with pytest.raises(pkg.srukf.SrukfError) as e:
        f.detect_features(img, block_size=7)
    assert e.value.rc == -6


def test_no_frame_held_is_a_sequence_error(synth, pkg):
    f = pkg.srukf.Filter(0, params(synth))
    with pytest.raises(pkg.srukf.SrukfError) as e:
        f.detect_features(None)
    assert e.value.rc == -5
    img = texture(8)
    uv1, _ = f.detect_features(img, unfiltered=True)
    uv2, _ = f.detect_features(None, unfiltered=True)    # the held frame
    assert np.array_equal(uv1, uv2)
    f.reset()
    with pytest.raises(pkg.srukf.SrukfError):
        f.detect_features(None)


def test_filter_map_gate(synth, pkg):
    f = pkg.srukf.Filter(0, params(synth))
    img = texture(11)
    kp = D.gftt(img, 60, 0.05, 10.0)
    near = [[kp[i, 0] + 3.0, kp[i, 1] + 2.0, 500.0, 400.0] for i in range(0, 20, 3)]
    for gate in (False, True):
        uv, _ = check_exact(f, img, max_corners=60, quality=0.05, min_dist=10.0, map_px=near, map_gate=gate)
        assert (len(uv) < len(D.filter_pass(kp, 640, 480, 10.0, 20.0)[0])) == gate
    zero = near + [[300.0, 0.0, 310.0, 200.0]]
    uv, _ = check_exact(f, img, max_corners=60, quality=0.05, min_dist=10.0, map_px=zero, map_gate=True)
    assert len(uv) == 0


def _archived_states(pkg, p, img, pose):
    """landmarks initialised at GFTT points of img under `pose`: their six state rows (FeatureInfo::state of an archived map)"""
    g = pkg.srukf.Filter(0, p)
    X4 = np.array(pose, dtype=np.float64)
    g.set_state(X4, np.diag([p["sigma_x"], p["sigma_y"], p["sigma_z"], p["sigma_theta"]]))
    kp = D.gftt(img, 6, 0.1, 15.0).astype(np.float64)
    g.add_landmarks(kp)
    X, _ = g.get_state()
    return X[:6 * len(kp)].reshape(-1, 6)


@pytest.mark.parametrize("project", [True, False])
def test_filter_archived(synth, pkg, project):
    p = params(synth)
    img = texture(12)
    pose = [0.3, -0.2, 0.0, 0.4]
    arch = _archived_states(pkg, p, img, pose)
    f = pkg.srukf.Filter(0, p)
    f.set_state(np.array(pose), np.diag([p["sigma_x"], p["sigma_y"], p["sigma_z"], p["sigma_theta"]]))
    if project:
        apx = pkg.srukf.project(p, arch, np.tile(pose[:3], (len(arch), 1)), np.full(len(arch), pose[3]), np.zeros((len(arch), 2)))
    else:
        apx = np.zeros((len(arch), 2))
    uv, loops = f.detect_features(img, max_corners=30, min_dist=15.0, archived=arch, project_archived=project)
    ruv, rloops = D.detect(img, 30, 0.1, 15.0, 3, 20, False, None, False, apx)
    assert np.array_equal(uv, ruv) and np.array_equal(loops, rloops)
    if project:
        assert len(loops) >= 3                          # the archived landmarks are seen again where they were created
    else:
        assert len(loops) == 0                          # (0, 0) is farther than min_dist from every key point inside the border
    # border 0: a key point near (0, 0) meets the unprojected archive
    img2 = np.zeros((480, 640), dtype=np.uint8)
    img2[4:40, 4:40] = 255
    uv, loops = f.detect_features(img2, max_corners=8, min_dist=10.0, border=0, archived=arch, project_archived=False)
    ruv, rloops = D.detect(img2, 8, 0.1, 10.0, 3, 0, False, None, False, np.zeros((len(arch), 2)))
    assert np.array_equal(uv, ruv) and np.array_equal(loops, rloops) and len(rloops) == len(arch)


def _host_cut(img, u, v):
    cu, cv = int(np.rint(u)), int(np.rint(v))
    return img[cv - 10:cv + 11, cu - 10:cu + 11]


def test_capture_appearance_matches_host_cut_patches(synth, pkg):
    p = params(synth)
    img = texture(21)
    img2 = np.roll(img, (1, 2), axis=(0, 1))
    S4 = np.diag([p["sigma_x"], p["sigma_y"], p["sigma_z"], p["sigma_theta"]])
    X4 = np.array([0.1, 0.05, 0.0, 0.3])
    fs = []
    for _ in range(3):
        f = pkg.srukf.Filter(0, p)
        f.set_state(X4, S4)
        fs.append(f)
    A, B, C = fs
    uv, _ = A.detect_features(img, max_corners=10, unfiltered=True)
    uv = uv + np.array([0.5, -0.5])                     # cvRound: half to even on both sides
    for f in fs:
        f.add_landmarks(uv)
    A.capture_appearance(0, uv)                         # the frame the detection left on the device: it survived add_landmarks
    C.capture_appearance(0, uv, img)
    pose, _ = B.get_robot()
    R = np.array([[math.cos(pose[3]), -math.sin(pose[3]), 0.0], [math.sin(pose[3]), math.cos(pose[3]), 0.0], [0.0, 0.0, 1.0]])
    for k in range(len(uv)):
        B.set_landmark_appearance(k, _host_cut(img, *uv[k]), R, pose[:3], uv[k])
    odo0, odo1 = np.array([0.0, 0.0, 0.0]), np.array([0.01, 0.004, 0.002])
    res = []
    for f in fs:
        f.predict_motion(odo0, odo1)
        f.predict_measurement()
        z, m, corr = f.associate(img2)
        res.append((z, m, corr, [f.get_match_patch(k) for k in range(len(uv))]))
    for other in res[1:]:
        assert np.array_equal(res[0][0], other[0]) and np.array_equal(res[0][1], other[1]) and np.array_equal(res[0][2], other[2])
        assert all(np.array_equal(a, b) for a, b in zip(res[0][3], other[3]))
    assert np.abs(res[0][2]).max() > 0.0
    with pytest.raises(pkg.srukf.SrukfError) as e:
        A.capture_appearance(0, [[5.0, 100.0]])         # the window leaves the image
    assert e.value.rc == -1


def _run_vision(tmp, frames, odo, *extra):
    H, W = frames[0].shape
    with open(os.path.join(tmp, "frames.bin"), "wb") as f:
        f.write(struct.pack("iii", W, H, len(frames)))
        for fr in frames:
            f.write(np.ascontiguousarray(fr, dtype=np.uint8).tobytes())
    with open(os.path.join(tmp, "odo.txt"), "w") as f:
        for i, (x, y, th) in enumerate(odo):
            f.write(f"{i + 1} : {0.1 * i:.3f} {float(x)!r} {float(y)!r} {float(th)!r}\n")
    out = subprocess.run([VISION, f"{tmp}/frames.bin", f"{tmp}/odo.txt", *extra], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def _parse(stdout):
    passes, frames, cur = [], [], None
    for line in stdout.splitlines():
        t = line.split()
        if not t:
            continue
        if t[0] == "pass":
            kv = dict(zip(t[1:-5:2], t[2:-5:2]))
            cur = {k: float(v) for k, v in kv.items()}
            cur["pose"] = [float(v) for v in t[-4:]]
            passes.append(cur)
        elif t[0] in ("map", "arch", "uv") and cur is not None and "loops" not in cur:
            cur[t[0]] = np.array([float(v) for v in t[1:]])
        elif t[0] == "loops":
            cur["loops"] = np.array([int(v) for v in t[1:]], dtype=np.int64).reshape(-1, 2)
        elif t[0] == "frame":
            frames.append({k: int(v) for k, v in zip(t[2::2], t[3::2])})
            frames[-1]["fr"] = int(t[1])
            frames[-1]["passes"] = passes[:]
            passes.clear()
            cur = None
        elif t[0] == "init":
            frames[-1]["init"] = np.array([float(v) for v in t[1:]]).reshape(-1, 2)
    return frames


def test_facade_detects_on_device(tmp_path, synth, pkg):
    assert os.path.exists(VISION), "run __graft_entry__.build() first"
    p = params(synth)
    base = texture(31)
    frames = [np.roll(base, (0, s), axis=(0, 1)) for s in range(4)]
    odo = [(0.01 * i, 0.0, 0.0) for i in range(7)]
    out = _run_vision(str(tmp_path), frames, odo, "redirect=3")
    recs = _parse(out)
    assert len(recs) == 5
    seen_proj = seen_frame1 = False
    for rec in recs:
        calls = {}
        for ps in rec["passes"]:
            calls.setdefault(int(ps["call"]), []).append(ps)
        last_uv = None
        for call, pl in sorted(calls.items()):
            first = pl[0]
            img = frames[int(first["image"])]
            proj = bool(first["proj"])
            arch = first["arch"].reshape(-1, 6)
            if proj and len(arch):
                pose = first["pose"]
                apx = pkg.srukf.project(p, arch, np.tile(pose[:3], (len(arch), 1)), np.full(len(arch), pose[3]), np.zeros((len(arch), 2)))
            else:
                apx = np.zeros((len(arch), 2))
            sched = D.add_features_schedule(img, int(first["frame"]), proj, bool(first["unf"]) and int(first["frame"]) != 1,
                                            int(first["n_map"]), int(first["n_matches"]), first["map"].reshape(-1, 4), apx)
            assert len(sched) == len(pl), (len(sched), len(pl))
            for s, ps in zip(sched, pl):
                assert s["max_corners"] == ps["mc"] and s["unfiltered"] == bool(ps["unf"]) and s["running"] == ps["running"]
                assert np.array_equal(s["uv"].ravel(), ps["uv"])
                assert np.array_equal(s["loops"], ps["loops"])
            seen_proj |= proj
            seen_frame1 |= int(first["frame"]) == 1
            last_uv = pl[-1]["uv"].reshape(-1, 2)
            n_map_after = int(first["n_map"]) + len(last_uv)
        assert rec["n_map"] == rec["map_size"] == len(rec["init"])          # m_nMapFeatures is the true map size
        if last_uv is not None and len(last_uv):
            assert rec["n_map"] == n_map_after
            assert np.array_equal(rec["init"][-len(last_uv):], last_uv)     # the new landmarks' init pixels are the key points
    assert seen_proj and seen_frame1
