"""GPU tests of the archive search (srukf_archive_set / srukf_archive_search, include/srukf.h) against the numpy restatement tests/np_archive.py.

PRED_TOL_H / PRED_TOL_P: stage (a) is compared with the restatement (the CPU oracle's projection, the device's order of sums) at 10 x the largest |dh| and
|d(Si^T Si)| measured on the MI355X over the cases of test_predict_equals_restatement (4.5e-13 px, 2.7e-13 px^2); both far below 1e-6.
Stages (b) and (c) are compared EXACTLY on the device's own h and Si: bytes, integers and one fp64 expression leave no room.
"""
import numpy as np
import pytest

import np_archive as A
from test_gpu_detect import texture

pytestmark = pytest.mark.gpu

PRED_TOL_H = 4.6e-12                                              # px   (largest seen: 4.547e-13, L = 5, the other step path, after the update of frame 3)
PRED_TOL_P = 2.8e-12                                              # px^2 (largest seen: 2.700e-13, L = 5, the other step path, frame 3 between predict and update)
F0 = 3
X4 = np.array([0.1, 0.05, 0.0, 0.0])
# where the reference's wrapPatch still produces the patch after the robot has moved 0.1 m to the left (restatement on the CPU: the warp holds in the cone of
# bearings the motion points along; elsewhere its template decays to a correlation of 0.3 - 0.6)
LEFT_UV = np.array([[70.0, 140.0], [70.0, 210.0], [70.0, 280.0], [140.0, 210.0], [140.0, 280.0]])
CORNER_UV = np.array([[14.0, 13.0], [626.0, 467.0]])                # 14 px inside: visible only for a record with little noise (test_windows_cut_by_the_image)


def params(synth):
    p = dict(synth.scene_params())
    p["image_w"], p["image_h"] = 640.0, 480.0
    return p


def S4_of(p, extra=(0.0, 0.0, 0.0, 0.0)):
    return np.diag(np.sqrt(np.array([p["sigma_x"], p["sigma_y"], p["sigma_z"], p["sigma_theta"]]) ** 2 + np.asarray(extra) ** 2))


def blob_frame(seed, UV):
    """test_gpu_detect.texture with a 45 x 45 block B = B^T centred on each pixel of UV (the reference's template is the transposed patch: tests/test_gpu_overlay.py)."""
    img = texture(seed).copy()
    rng = np.random.default_rng(seed)
    for u, v in np.asarray(UV).astype(int):
        R = rng.integers(0, 256, size=(49, 49)).astype(np.float64)
        c = np.cumsum(np.cumsum(R, 0), 1)
        R = (c[4:, 4:] - c[:-4, 4:] - c[4:, :-4] + c[:-4, :-4]) / 16.0
        y0, y1, x0, x1 = max(v - 22, 0), min(v + 23, 480), max(u - 22, 0), min(u + 23, 640)
        img[y0:y1, x0:x1] = (0.5 * (R + R.T)).astype(np.uint8)[y0 - (v - 22):y1 - (v - 22), x0 - (u - 22):x1 - (u - 22)]
    return img


def capture_records(srukf, p, img, UV, S4=None):
    """Landmarks created at UV of img from the robot state (X4, default S4), appearance captured; returns their records (arrays) and the filter, emptied again."""
    f = srukf.Filter(0, p)
    f.set_state(X4, S4_of(p) if S4 is None else S4)
    f.add_landmarks(UV)
    f.capture_appearance(0, UV, img)
    recs = [f.get_landmark_record(k) for k in range(len(UV))]
    assert all(r["has_app"] for r in recs)
    for _ in range(len(UV)):
        f.delete_landmark(0)
    assert f.N == 0
    rec = {k: np.array([r[k] for r in recs]) for k in ("X6", "S66", "patch", "R", "t", "px")}
    return rec, f


def set_archive(f, rec, idx=None):
    idx = np.arange(len(rec["X6"])) if idx is None else np.asarray(idx)
    f.archive_set(rec["X6"][idx], rec["S66"][idx], rec["patch"][idx], rec["R"][idx], rec["t"][idx], rec["px"][idx])


def check_chain(f, oracle, p, rec, img, res, half_cap):
    """Stages (b) and (c) of the device against the restatement fed with the device's h, Si and visible: templates byte for byte, z / matched / corr exactly."""
    h, Si, vis, z, m, cr = res
    L = len(vis)
    pose, _ = f.get_robot()
    _, _, _, xyz, _ = A.predict(oracle, p, rec["X6"], rec["S66"], pose, np.zeros((4, 4)))
    tm = A.warp(oracle, p, pose, rec["patch"], rec["R"], rec["t"], rec["px"], xyz, h.reshape(L, 2), vis)
    for k in range(L):
        assert np.array_equal(f.archive_template(k), tm[k]), k
    z2, m2, cr2 = A.search(p, img, h.reshape(L, 2), Si, vis, tm, half_cap)
    assert np.array_equal(m, m2), (m, m2)
    assert np.array_equal(cr, cr2), (cr, cr2)
    assert np.array_equal(z.reshape(L, 2), z2)
    return tm


def _warm_state(srukf, sc, N, p):
    f = srukf.Filter(N, p); f.set_state(sc["X0"], sc["S0"]); f.stage_sequence(sc["odo"], sc["z"], sc["matched"])
    f.run_frames(0, F0)
    X, S = f.get_state(); f.close()
    return X, S


def _predict(f, sc, t, fast):
    f.predict_motion(sc["odo"][t], sc["odo"][t + 1])
    if fast:
        f.predict_motion_next(sc["odo"][t + 1], sc["odo"][t + 2])
    return f.predict_measurement()


def scene_records(f, ks, far=False):
    """Records of landmarks ks of a running filter (they have no appearance: a flat patch, the identity view); far: one more whose anchor lies 50 m aside."""
    recs = [f.get_landmark_record(int(k)) for k in ks]
    X6 = np.array([r["X6"] for r in recs]); S66 = np.array([r["S66"] for r in recs])
    if far:
        X6 = np.vstack([X6, X6[0] + np.array([50.0, 0, 0, 0, 0, 0])]); S66 = np.concatenate([S66, S66[:1]])
    L = len(X6)
    return {"X6": X6, "S66": S66, "patch": np.full((L, 21, 21), 100, dtype=np.uint8), "R": np.tile(np.eye(3), (L, 1, 1)), "t": np.zeros((L, 3)),
            "px": np.tile([320.0, 240.0], (L, 1))}


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("L", [1, 5])
def test_predict_equals_restatement(srukf, synth, oracle, L, fast):
    """Stage (a): h, Si^T Si and visible of the device against the restatement fed get_robot()'s pose and P4, a few frames into a filter (P4 is a real covariance),
    after an update and between predict_measurement and update, on both step paths.  (N = 50, seed 11: with the restatement on the CPU every sigma pixel of the
    records used lies more than 80 px from a validity border; the record 50 m aside has all 25 zeroed.)"""
    N, seed = 50, 11
    p = synth.scene_params()
    sc = synth.make_scene(N, F0 + 5, seed=seed, p=p)
    X3, S3 = _warm_state(srukf, sc, N, p)
    f = srukf.Filter(N, p); f.set_state(X3, S3); f.debug_set("step_fast", fast)
    img = texture(4, H=int(p["image_h"]), W=int(p["image_w"]))
    ks = [7] if L == 1 else [3, 12, 20, 41]
    worst_h = worst_p = 0.0
    for t in range(F0, F0 + 2):
        h0, Si0, vis0 = _predict(f, sc, t, fast)
        for phase in ("between", "after"):
            if phase == "after":
                f.update(sc["z"][t], sc["matched"][t])
            rec = scene_records(f, ks, far=(L == 5))
            set_archive(f, rec)
            assert f.archive_count() == L
            h, Si, vis, z, m, cr = f.archive_search(img)
            pose, P4 = f.get_robot()
            hr, Sir, visr, _, Z = A.predict(oracle, p, rec["X6"], rec["S66"], pose, P4)
            assert all(A.border_margin(p, Z[k]) > 1.0 for k in range(len(ks)))
            assert np.array_equal(vis, visr) and vis[:len(ks)].all() and (L == 1 or vis[-1] == 0)
            v = vis != 0
            dh = np.abs(h.reshape(L, 2) - hr)[v].max()
            Pd = np.einsum("kab,kac->kbc", Si, Si); Pr = np.einsum("kab,kac->kbc", Sir, Sir)
            dp = np.abs(Pd - Pr)[v].max()
            print(f"archive predict L={L} fast={fast} t={t} {phase}: max|dh| = {dh:.3e} px, max|d(Si^T Si)| = {dp:.3e} px^2")
            worst_h, worst_p = max(worst_h, dh), max(worst_p, dp)
            assert (Si[:, 1, 0] == 0.0).all()
            if L == 5:
                assert m[-1] == 0 and cr[-1] == 0.0 and z[-2] == 0.0 and z[-1] == 0.0 and not f.archive_template(L - 1).any()
    assert f.debug_get("step_fast") == (2 if fast else 0)
    assert worst_h <= PRED_TOL_H and worst_p <= PRED_TOL_P, (worst_h, worst_p)
    f.close()


@pytest.mark.parametrize("half_cap", [10, 40])
def test_windows_cut_by_the_image(srukf, synth, oracle, half_cap):
    """A record whose staged region is cut by the left and top edges of the image and one cut by the right and bottom edges: device == restatement, exactly.
    (14 px inside the image the 25 sigma pixels stay valid only for a sharp record: pixel noise 0.5 px, a robot and a record known to a millimetre.)"""
    p = params(synth)
    p["sigma_measure"] = 0.5
    img = blob_frame(5, CORNER_UV)
    S4 = 1e-3 * np.eye(4)
    rec, f = capture_records(srukf, p, img, CORNER_UV, S4)
    rec["S66"] = rec["S66"] * 0.02
    f.set_state(X4, S4)
    set_archive(f, rec)
    res = f.archive_search(img, half_cap=half_cap)
    check_chain(f, oracle, p, rec, img, res, half_cap)
    h, Si, vis, z, m, cr = res
    print("corner records: matched", m, "corr", np.round(cr, 3))
    assert vis.tolist() == [1, 1]
    hx, hy, x0, y0, _ = A.window(h.reshape(2, 2)[0], Si[0], half_cap)
    assert x0 - 8 < 0 and y0 - 8 < 0                             # the staged region leaves the image on the left and at the top
    hx, hy, x0, y0, _ = A.window(h.reshape(2, 2)[1], Si[1], half_cap)
    assert x0 + 2 * hx + 8 > 639 and y0 + 2 * hy + 8 > 479      # ... on the right and at the bottom
    f.close()


@pytest.mark.parametrize("half_cap", [10, 40])
def test_warp_and_search_equal_restatement(srukf, synth, oracle, half_cap):
    """Stages (b) and (c) chained on the device's own outputs, and what each case must find.  The records' patches lie ~26 px from h once the robot state has
    moved 0.1 m: found at cap 40, not at cap 10."""
    p = params(synth)
    UV = LEFT_UV
    img = blob_frame(5, UV)
    rec, f = capture_records(srukf, p, img, UV)
    # the identity view: every patch at its pixel
    f.set_state(X4, S4_of(p))
    set_archive(f, rec, [0, 3, 4])
    sub = {k: v[[0, 3, 4]] for k, v in rec.items()}
    res = f.archive_search(img, half_cap=half_cap)
    check_chain(f, oracle, p, sub, img, res, half_cap)
    h, Si, vis, z, m, cr = res
    assert vis.tolist() == [1, 1, 1] and m.tolist() == [1, 1, 1] and (cr > 0.99).all()
    assert np.array_equal(z.reshape(3, 2), UV[[0, 3, 4]] + 1.0)  # (the reference's template is cut one pixel off-centre: tests/test_gpu_parity.py)
    # a patch absent from the frame
    res = f.archive_search(texture(5), half_cap=half_cap)
    check_chain(f, oracle, p, sub, texture(5), res, half_cap)
    assert res[4].tolist() == [0, 0, 0] and (res[5] <= 0.8).all() and not res[3].any()
    # the robot state 0.1 m to the left, P4 inflated accordingly: the patches lie ~26 px from h, inside the gate
    d = np.array([-0.1, 0.0, 0.0, 0.0])
    f.set_state(X4 + d, S4_of(p, np.abs(d)))
    set_archive(f, rec, [0, 1, 2, 3, 4])
    sub = {k: v[:5] for k, v in rec.items()}
    res = f.archive_search(img, half_cap=half_cap)
    check_chain(f, oracle, p, sub, img, res, half_cap)
    h, Si, vis, z, m, cr = res
    dist = np.hypot(*(h.reshape(5, 2) - LEFT_UV).T)
    print("patch distance from h", np.round(dist, 1), "corr", np.round(cr, 3))
    assert vis.all() and (dist > 20).all() and (dist < 30).all()
    if half_cap == 40:
        assert m.all() and np.array_equal(z.reshape(5, 2), LEFT_UV + 1.0)
    else:
        assert not m.any() and (cr <= 0.8).all()
    # in the box, outside the gate ellipse: the frame moved by (20, 30) under an ellipse that is long in y only (identity view, P4 inflated in x alone)
    f.set_state(X4, S4_of(p, (0.1, 0.0, 0.0, 0.0)))
    set_archive(f, rec, [3])
    sub = {k: v[[3]] for k, v in rec.items()}
    moved = np.roll(img, (30, 20), axis=(0, 1))
    res = f.archive_search(moved, half_cap=40)
    check_chain(f, oracle, p, sub, moved, res, 40)
    h, Si, vis, z, m, cr = res
    hx, hy, x0, y0, (i00, i01, i10, i11) = A.window(h, Si[0], 40)
    e = UV[3] + 1.0 + np.array([20.0, 30.0]) - h
    assert abs(e[0]) <= hx and abs(e[1]) <= hy and (e[0] * i00 + e[1] * i10) * e[0] + (e[0] * i01 + e[1] * i11) * e[1] >= A.CHI2
    assert vis[0] == 1 and m[0] == 0 and cr[0] <= 0.8
    cc, _, _ = A.scores(moved, h, Si[0], f.archive_template(0), 40, chi2=1e9)          # ... and it IS there for a gate that lets it through
    assert cc.max() > 0.99
    f.close()


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("fast", [0, 1])
def test_search_is_read_only(srukf, synth, fast, storage):
    """Two filters over the same frames; one searches the archive after every update and once between predict_measurement and update: X and S bit-identical
    after every frame (the fast path's chain and what its updates submit ahead included)."""
    N, seed = 50, 11
    p = synth.scene_params()
    sc = synth.make_scene(N, F0 + 6, seed=seed, p=p)
    X3, S3 = _warm_state(srukf, sc, N, p)
    img = texture(4, H=int(p["image_h"]), W=int(p["image_w"]))
    out = []
    for with_search in (0, 1):
        f = srukf.Filter(N, p)
        if storage == "f32":
            f.set_storage(srukf.STORAGE_F32)
        f.set_state(X3, S3); f.debug_set("step_fast", fast)
        if with_search:
            set_archive(f, scene_records(f, [3, 12, 20, 41], far=True))
        states = []
        for t in range(F0, F0 + 4):
            h, Si, vis = _predict(f, sc, t, fast)
            if with_search and t == F0 + 1:
                r = f.archive_search(img)
                assert r[2][:4].all()
                h2, Si2, vis2 = f.predict_measurement()          # (the statistics the host sees are untouched)
                assert np.array_equal(h, h2) and np.array_equal(Si, Si2) and np.array_equal(vis, vis2)
            f.update(sc["z"][t], sc["matched"][t])
            if with_search:
                r = f.archive_search(img if t == F0 else None)   # (the held frame from then on)
                assert r[2][:4].all() and r[2][4] == 0
            states.append(f.get_state() + (f.get_state_f32() if storage == "f32" else (0, 0)))
        out.append((states, f.debug_get("step_fast")))
        f.close()
    assert out[0][1] == out[1][1] == (4 if fast else 0)
    for a, b in zip(out[0][0], out[1][0]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_lifetime_and_errors(srukf, synth, oracle):
    p = params(synth)
    UV = LEFT_UV[:3]
    img = blob_frame(5, UV)
    rec, f = capture_records(srukf, p, img, UV)                  # (the filter has been through N = 3 .. 0: retired contexts exist)
    assert f.archive_count() == 0
    with pytest.raises(srukf.SrukfError) as e:
        f.archive_template(0)
    assert e.value.rc == -1
    f.archive_search(img)                                         # an empty archive: nothing to do, the frame is taken
    set_archive(f, rec)
    assert f.archive_count() == 3 and not f.archive_template(1).any()                  # zeros before any search
    r0 = f.archive_search(None)
    assert r0[2].all() and r0[4].any()
    t0 = [f.archive_template(k) for k in range(3)]
    rob0 = f.get_robot()

    def discrete_same(r, what):
        for q in (2, 3, 4, 5):
            assert np.array_equal(r[q], r0[q]), (what, q)
        assert all(np.array_equal(f.archive_template(k), t0[k]) for k in range(3)), what

    # A map change that leaves the pose alone: srukf_insert_landmarks copies X and S, so the pose and P4 keep their bits (asserted) and the search must return
    # every output bit for bit.
    f.insert_landmarks(rec["X6"][:1], rec["S66"][:1])
    assert f.N == 1 and f.archive_count() == 3
    rob1 = f.get_robot()
    assert np.array_equal(rob1[0], rob0[0]) and np.array_equal(rob1[1], rob0[1])
    r1 = f.archive_search(None)
    assert all(np.array_equal(a, b) for a, b in zip(r0, r1))
    discrete_same(r1, "insert_landmarks")
    # srukf_add_landmarks and srukf_delete_landmark (revived contexts) factor S again: the archive survives, and the search is the search of the robot block as
    # it then is: visible, z, matched, corr and the templates as before, exactly; h and Si^T Si against the restatement fed get_robot() then, at stage (a)'s bound.
    def survives(what):
        assert f.archive_count() == 3
        r = f.archive_search(None)
        pose, P4 = f.get_robot()
        assert np.array_equal(pose, rob0[0]), what
        hr, Sir, visr, _, _ = A.predict(oracle, p, rec["X6"], rec["S66"], pose, P4)
        dh = np.abs(r[0].reshape(3, 2) - hr).max()
        dP = np.abs(np.einsum("kab,kac->kbc", r[1], r[1]) - np.einsum("kab,kac->kbc", Sir, Sir)).max()
        print(f"archive after {what}: max|dP4| = {np.abs(P4 - rob0[1]).max():.3e}, against the restatement max|dh| = {dh:.3e}, max|dPi| = {dP:.3e}")
        assert np.array_equal(r[2], visr) and dh <= PRED_TOL_H and dP <= PRED_TOL_P, (what, dh, dP)
        discrete_same(r, what)

    f.add_landmarks(np.array([[300.0, 200.0], [400.0, 260.0]]))
    assert f.N == 3
    survives("add_landmarks")
    f.delete_landmark(2); f.delete_landmark(1)
    assert f.N == 1                                               # (N = 1: the context the insertion left behind, revived)
    survives("delete_landmark")
    # refused
    bad = {k: v.copy() for k, v in rec.items()}
    bad["S66"][1, 4, 2] = 1e-3
    for args, rc in (((bad["X6"], bad["S66"], bad["patch"], bad["R"], bad["t"], bad["px"]), -1),
                     ((rec["X6"] * np.nan, rec["S66"], rec["patch"], rec["R"], rec["t"], rec["px"]), -1),
                     ((rec["X6"], rec["S66"], rec["patch"], rec["R"], rec["t"] + np.inf, rec["px"]), -1)):
        with pytest.raises(srukf.SrukfError) as e:
            f.archive_set(*args)
        assert e.value.rc == rc
    lib = srukf.load_library()
    import ctypes as C
    x6 = np.ascontiguousarray(rec["X6"]); dp = C.POINTER(C.c_double)
    assert lib.srukf_archive_set(f._h, -1, None, None, None, None, None, None) == -1
    assert lib.srukf_archive_set(f._h, 3, x6.ctypes.data_as(dp), None, None, None, None, None) == -1
    assert f.archive_count() == 3                                 # a refused call leaves the archive as it was
    for cap in (9, 41):
        with pytest.raises(srukf.SrukfError) as e:
            f.archive_search(None, half_cap=cap)
        assert e.value.rc == -1
    assert lib.srukf_archive_search(f._h, None, None, None, None, None, None, None, None) == 0      # NULL params: the defaults; every output may be NULL
    # L = 0 clears; reset drops the archive and the held frame
    f.archive_set(np.zeros((0, 6)), np.zeros((0, 6, 6)), np.zeros((0, 21, 21), dtype=np.uint8), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros((0, 2)))
    assert f.archive_count() == 0
    set_archive(f, rec)
    f.reset()
    assert f.archive_count() == 0
    with pytest.raises(srukf.SrukfError) as e:
        f.archive_search(None)
    assert e.value.rc == -5
    f.close()


def test_end_to_end_reinsertion(srukf, synth, oracle):
    """Landmarks captured on a texture, archived, the robot state then drifts 0.1 m (projections move ~26 px: beyond m_minDist = 15 px, the reference's geometric
    test cannot fire) with P4 inflated accordingly; the same frame (the robot has not moved in truth) is searched.  Every record is matched within 1 px of its
    projection from the true pose.  All of them go back (srukf_insert_landmarks) and the next frame is predicted, associated and updated as CSLAM does it with
    searchArchivedLandmarks on: the ordinary association looks +- 10 px around predictions ~26 px off (HP_INIT, SLAM.cpp:1955-1956), so the nodes it leaves
    unmatched are looked for once more, in the next frame, with the search's window (their records are still on the device), and measured one at a time,
    predicted again from the posterior in between (the reference's update sums the gains of one prior: five landmarks that agree on 26 px overshoot together,
    0.1 m -> 0.26 m).  The pose error shrinks with every one of them."""
    p = params(synth)
    img = blob_frame(5, LEFT_UV)
    rec, f = capture_records(srukf, p, img, LEFT_UV)
    L = len(LEFT_UV)
    d = np.array([-0.1, 0.0, 0.0, 0.0])
    f.set_state(X4 + d, S4_of(p, np.abs(d)))
    set_archive(f, rec)
    h, Si, vis, z, m, cr = f.archive_search(img)
    true_px = oracle.project(p, rec["X6"], np.tile(X4[:3], (L, 1)), np.full(L, X4[3]), np.zeros((L, 2)))
    shift = np.hypot(*(h.reshape(L, 2) - true_px).T)
    print("shift", np.round(shift, 1), "corr", np.round(cr, 3), "z - true", np.round(z.reshape(L, 2) - true_px, 3).tolist())
    assert (shift > 20).all() and (shift < 30).all()
    assert vis.all() and m.all()
    assert np.abs(z.reshape(L, 2) - true_px).max() <= 1.0         # (the reference's template is cut one pixel off-centre: 0.993 on the CPU restatement)
    f.insert_landmarks(rec["X6"], rec["S66"], rec["patch"], rec["R"], rec["t"], rec["px"])
    assert f.N == L and f.archive_count() == L
    err = [np.abs(f.get_robot()[0] - X4)[:2].max()]
    # the next frame (the robot at rest, the same picture)
    f.predict_motion(np.zeros(3), np.zeros(3))
    hp, Sip, visp = f.predict_measurement()
    za, ma, _ = f.associate(img)
    h2, Si2, vis2, z2, m2, _ = f.archive_search(None)             # the frame the association uploaded
    print("ordinary association matched", ma.tolist(), "second search matched", m2.tolist())
    assert visp.all() and ((ma != 0) | (m2 != 0)).all()
    assert np.abs(z2.reshape(L, 2)[m2 != 0] - true_px[m2 != 0]).max() <= 1.0
    zz = np.where(np.repeat(ma, 2) != 0, za, z2)
    updated = False
    if ma.any():
        f.update(zz, ma); updated = True
        err.append(np.abs(f.get_robot()[0] - X4)[:2].max())
    for k in np.flatnonzero(ma == 0):
        if updated:
            hk, Sik, visk = f.repredict_measurement()
            y = np.linalg.solve(Sik[k].T, zz[2 * k:2 * k + 2] - hk[2 * k:2 * k + 2])
            assert visk[k] and y @ y < 5.99146454710798, (k, y @ y)      # dataAssociation's gate (1977) at the prediction from the posterior
        one = np.zeros(L, dtype=np.int32); one[k] = 1
        f.update(zz, one); updated = True
        err.append(np.abs(f.get_robot()[0] - X4)[:2].max())
    print("pose error, m:", " -> ".join(f"{e:.4f}" for e in err))
    assert abs(err[0] - 0.1) < 1e-12 and len(err) >= 2
    assert all(b < a for a, b in zip(err, err[1:])) and err[-1] < 0.25 * err[0]
    f.close()


def _archive_lines(out):
    recs = []
    for line in out.splitlines():
        t = line.split()
        if t[:1] == ["archive"]:
            kv = {k: int(v) for k, v in zip(t[1:13:2], t[2:13:2])}
            kv["ids"] = [int(v) for v in t[14:]]
            recs.append(kv)
    return recs


def test_facade_searches_the_archive(tmp_path):
    """cslam_vision redirect=3 loops archive=40: the restart archives the map and the search finds it again in the restart's frame.  Every landmark put back keeps
    its ID with isLoop set, archive and map move by the same count, m_nArchiveMatches counts them, the geometric loop points of the restart's pass are left to the
    search's verdict (none goes back twice), and the nodes put back are measured in that frame.  Without archive= the switch's lines are absent and the run is the
    `loops` run; up to the restart the switch changes nothing the host sees."""
    import os
    from test_gpu_detect import VISION, _run_vision
    from test_gpu_loop import _vision_records
    assert os.path.exists(VISION), "run __graft_entry__.build() first"
    base = texture(31)
    frames = [np.roll(base, (0, s), axis=(0, 1)) for s in range(4)]
    odo = [(0.01 * i, 0.0, 0.0) for i in range(7)]
    off = _run_vision(str(tmp_path), frames, odo, "redirect=3", "loops")
    out = _run_vision(str(tmp_path), frames, odo, "redirect=3", "archive=40")
    mine = (["archive"], ["reacquired"], ["archive_matches"])
    assert not any(line.split()[:1] in mine for line in off.splitlines())
    recs, reins = _vision_records("\n".join(line for line in out.splitlines() if line.split()[:1] not in mine))
    searches = _archive_lines(out)
    put_back = [a for a in searches if a["ids"]]
    assert len(reins) == 1 and len(put_back) >= 1
    fr = reins[0]["frame"]
    # up to the restart nothing is archived with a record: the two runs print the same lines
    cut = [i for i, line in enumerate(off.splitlines()) if line.startswith("frame ")][fr - 1] + 4       # (frame, init, ids, pose)
    assert [l for l in out.splitlines() if l.split()[:1] not in mine][:cut] == off.splitlines()[:cut]
    before = set()
    for r in recs[:fr]:
        before |= set(r["ids"][:, 0].tolist())
    total = 0
    for a in put_back:
        n = len(a["ids"])
        total += n
        assert a["n_after"] - a["n_before"] == n and a["archived_before"] - a["archived_after"] == n      # archive and map move by the same count
        assert a["searched"] >= n
    first = put_back[0]
    assert set(first["ids"]) <= before and first["n_before"] == 0   # the restart's search, in front of its addFeatures: the map it left behind, found again
    ids = recs[fr]["ids"]
    loops = ids[ids[:, 1] == 1, 0].tolist()
    assert loops and set(loops) <= set(first["ids"])                # ID kept, isLoop set (the deletion policy may have removed some since)
    assert loops == [i for i in first["ids"] if i in loops] and ids[:len(loops), 1].all()
    assert reins[0]["ids"] == []                                     # the geometric loop points of the restart's pass: the search had its say, none goes back by them
    for r in recs:
        assert len(set(r["ids"][:, 0].tolist())) == len(r["ids"])    # no ID twice in a map
    tail = dict(zip(out.splitlines()[-2].split()[0::2], out.splitlines()[-2].split()[1::2]))
    assert int(tail["archive_matches"]) == total
    last = [ps for ps in recs[fr]["passes"] if int(ps["call"]) == reins[0]["call"]][-1]
    assert int(tail["archive_rejected"]) == len(set(last["loops"][:, 1].tolist()))     # what the restart's last pass met and the search had not matched stays archived
    reacq = [int(l.split()[1]) for l in out.splitlines() if l.startswith("reacquired ")]
    assert len(reacq) == len(recs) and sum(reacq) == int(tail["archive_reacquired"])
    print("archive searches:", searches, "reacquired per frame:", reacq, "tail:", tail)
