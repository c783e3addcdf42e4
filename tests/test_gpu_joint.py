"""GPU tests of the joint measurement update (srukf_update_joint, csrc/srukf_joint.hip) against its numpy restatement (tests/np_joint.py).
Shapes sit at the panel boundaries of the new kernels (64-row panels of the 2N x 2N innovation covariance): N = 8 (one panel), N = 33 (two, two real rows in
the second), N = 70 (three).  Bounds: the project's per-frame |dX| <= 1e-9, |dP| <= 1e-11; for the shipped constants the larger of those and 10 x the
restatement's float64-vs-longdouble floor (np_joint.shipped_tolerance: the floor is ~1e-15, so the same numbers)."""
import functools

import numpy as np
import pytest

import np_joint as J

pytestmark = pytest.mark.gpu

TOL_X, TOL_P = 1e-9, 1e-11


def mask(kind, N):
    m = np.ones(N, dtype=np.int32)
    if kind == "alt": m[1::2] = 0
    elif kind == "first32": m[:32] = 0
    elif kind == "one": m[:] = 0; m[N // 2] = 1
    return m


def params_of(synth, which):
    return synth.scene_params() if which == "scene" else synth.default_params()


@functools.lru_cache(maxsize=None)
def _scene(synth, N, which, F=4):
    return synth.make_scene(N, F, seed=3, p=params_of(synth, which))


@functools.lru_cache(maxsize=None)
def _shipped_tol(synth):
    return J.shipped_tolerance(synth, 8, 20)


def tol(synth, which):
    return (TOL_X, TOL_P) if which == "scene" else _shipped_tol(synth)


def start(srukf, sc, oov=None, fast=None, X0=None, S0=None):
    """a device filter on the scene's initial state; oov: that landmark's bearing turned 1.2 rad, every sigma point of it leaves the image (they all project to the
    same pixel: h != 0, Si = 0 — inactive by its singular Si)"""
    X0 = (sc["X0"] if X0 is None else X0).copy()
    if oov is not None: X0[6 * oov + 3] += 1.2
    f = srukf.Filter(sc["N"], sc["params"]); f.set_state(X0, sc["S0"] if S0 is None else S0)
    if fast is not None: f.debug_set("step_fast", fast)
    return f, X0


def dims(f):
    return (f.n + 63) // 64 * 64, (2 * f.N + 63) // 64 * 64


CASES = [(8, "all", None, "scene"), (8, "alt", None, "scene"), (8, "one", None, "scene"), (8, "all", 5, "scene"), (33, "all", None, "scene"), (33, "first32", None, "scene"),
         (33, "alt", 32, "scene"), (70, "all", None, "scene"), (70, "alt", None, "scene"), (70, "one", None, "scene"), (8, "all", None, "shipped"), (33, "all", None, "shipped")]


@pytest.mark.parametrize("N,kind,oov,which", CASES)
def test_kernel_stage_R_and_Ut(srukf, synth, N, kind, oov, which):
    """R and U^T as the kernels leave them (srukf_debug_copy "joint_R", "Ut") against np_joint.joint_arrays fed the device's own Z, h, prior X / S and
    the cross covariance k_gain would have read (wi gamma S^T DZ, PxyR); the second frame of the scene, so the prior is the filter's own."""
    sc = _scene(synth, N, which)
    f, _ = start(srukf, sc, oov, fast=0)
    m = mask(kind, N)
    f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement(); f.update_joint(sc["z"][0], m)
    f.predict_motion(sc["odo"][1], sc["odo"][2]); h, Si, vis = f.predict_measurement()
    if oov is not None: assert np.all(Si[oov] == 0) and vis.sum() == N
    X, S = f.get_state()
    f.update_joint(sc["z"][1], m)
    n, Na, L = f.n, f.Na, f.L
    np_, mp = dims(f)
    ldw = mp + np_ + 32
    Z = f.debug_copy("Z", L * mp).reshape(L, mp)[:, :2 * N].T.copy()
    DZ = f.debug_copy("DZ", np_ * mp).reshape(np_, mp)
    PxyR = f.debug_copy("PxyR", 5 * mp).reshape(5, mp)
    _, _, wi, _, gamma = synth.ut_weights(Na, sc["params"]["weight_type"], sc["params"]["ut_alpha"], sc["params"]["ut_beta"])
    Pxy = np.vstack([wi * gamma * (S[:n, :n - 4].T @ DZ[:n, :2 * N]), PxyR[:4, :2 * N]])
    act = (m != 0) & (vis != 0) & (J.si_det(Si) != 0)
    if oov is not None and m[oov]: assert not act[oov] and act.sum() == m.sum() - 1
    ref = J.joint_arrays(Z, h, X, S, Pxy, sc["z"][1], act, wi, n, Na)
    W = f.debug_copy("joint_R", mp * ldw).reshape(mp, ldw)
    Ut = f.debug_copy("Ut", mp * np_).reshape(mp, np_)
    X2, S2 = f.get_state()
    f.close()
    dR, dU = np.abs(W[:2 * N, :2 * N] - ref["R"]).max(), np.abs(Ut[:2 * N, :n] - ref["Ut"]).max()
    Sref = J.gmw(ref["G"], sc["params"]["epsilon"])[0]
    dX, dP = np.abs(X2 - ref["X"]).max(), np.abs(S2.T @ S2 - Sref.T @ Sref).max()
    print("N=%d %s oov=%s %s: |dR| %.2e |dUt| %.2e |dX| %.2e |dP| %.2e  cond(Pzz) %.3g" % (N, kind, oov, which, dR, dU, dX, dP, np.linalg.cond(ref["Pzz"])))
    tx, tp = tol(synth, which)
    # the padding rows of the work matrix: identity in R, zero in U^T; nothing below R's diagonal; U^T rows of inactive landmarks zero
    assert np.array_equal(W[2 * N:, :mp], np.eye(mp)[2 * N:]) and np.array_equal(np.tril(W[:, :mp], -1), np.zeros((mp, mp)))
    assert np.array_equal(Ut[2 * N:], np.zeros((mp - 2 * N, np_))) and np.array_equal(Ut[:2 * N][~np.repeat(act, 2)], np.zeros((2 * int((~act).sum()), np_)))
    assert np.array_equal(W[:, mp:mp + np_], Ut)
    assert dR <= tx and dU <= tp and dX <= tx and dP <= tp


@pytest.mark.parametrize("N,kind,oov,which", [(8, "all", None, "scene"), (8, "alt", 4, "scene"), (33, "first32", None, "scene"), (33, "all", None, "shipped"), (70, "all", None, "scene")])
def test_filter_stage_three_frames(srukf, synth, N, kind, oov, which):
    """X and S^T S after update_joint against NpJointFilter.update_joint, three frames from the same initial state"""
    sc = _scene(synth, N, which)
    f, X0 = start(srukf, sc, oov)
    g = J.NpJointFilter(N, sc["params"], synth); g.set_state(X0, sc["S0"])
    m = mask(kind, N)
    tx, tp = tol(synth, which)
    worst = [0.0, 0.0]
    for t in range(3):
        f.predict_motion(sc["odo"][t], sc["odo"][t + 1]); h, Si, vis = f.predict_measurement()
        g.predict_motion(sc["odo"][t], sc["odo"][t + 1]); g.predict_measurement()
        assert np.array_equal((vis != 0) & (J.si_det(Si) != 0), g.active(np.ones(N)))
        if oov is not None: assert not g.active(np.ones(N))[oov]
        f.update_joint(sc["z"][t], m); g.update_joint(sc["z"][t], m)
        X, S = f.get_state()
        worst = [max(worst[0], np.abs(X - g.X).max()), max(worst[1], np.abs(S.T @ S - g.S.T @ g.S).max())]
    assert f.clamp_info() == (-1, -1)
    f.close()
    print("N=%d %s oov=%s %s: |dX| %.2e |dP| %.2e" % (N, kind, oov, which, *worst))
    assert worst[0] <= tx and worst[1] <= tp


@pytest.mark.parametrize("N", [8, 70])
def test_one_active_landmark_equals_batched(srukf, synth, N):
    """With one active landmark the joint update is the reference's update for that landmark: a twin that runs update(mode = BATCHED)"""
    sc = _scene(synth, N, "scene")
    m = mask("one", N)
    out = []
    for joint in (True, False):
        f, _ = start(srukf, sc)
        for t in range(2):
            f.predict_motion(sc["odo"][t], sc["odo"][t + 1]); f.predict_measurement()
            f.update_joint(sc["z"][t], m) if joint else f.update(sc["z"][t], m, mode=srukf.UPDATE_BATCHED)
        X, S = f.get_state(); out.append((X, S.T @ S)); f.close()
    dX, dP = np.abs(out[0][0] - out[1][0]).max(), np.abs(out[0][1] - out[1][1]).max()
    print("N=%d: |dX| %.2e |dP| %.2e" % (N, dX, dP))
    assert dX <= TOL_X and dP <= TOL_P


def test_need_reorder_behind_an_addition(srukf, synth):
    """N = 8 -> 10 by add_landmarks, then the NEED_REORDER joint frame: np_joint followed by the restatement's reorder factorisation on S^T S - U U^T.
    And a NEEDNOT_REORDER joint frame leaves the number of null directions as it was."""
    sc = _scene(synth, 8, "scene")
    f, _ = start(srukf, sc)
    f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement()
    nd = f.null_directions()
    f.update_joint(sc["z"][0], sc["matched"][0])
    assert f.null_directions() == nd
    f.add_landmarks(np.array([[300.0, 200.0], [350.0, 260.0]]))
    assert f.N == 10
    X, S = f.get_state()
    g = J.NpJointFilter(10, sc["params"], synth); g.set_state(X, S)
    f.predict_motion(sc["odo"][1], sc["odo"][2]); h, Si, vis = f.predict_measurement()
    g.predict_motion(sc["odo"][1], sc["odo"][2]); g.predict_measurement()
    rng = np.random.default_rng(11)
    z = h + rng.normal(0, 0.3, h.shape); m = np.asarray(vis, dtype=np.int32)
    assert m.sum() == 10
    f.update_joint(z, m, reorder=srukf.NEED_REORDER)
    o = g.joint(z, m)
    P = J.reorder_refactor(o["G"], 2, sc["params"]["epsilon"], synth)
    X2, S2 = f.get_state(); f.close()
    dX, dP = np.abs(X2 - o["X"]).max(), np.abs(S2.T @ S2 - P).max()
    print("NEED_REORDER: |dX| %.2e |dP| %.2e" % (dX, dP))
    assert dX <= TOL_X and dP <= TOL_P


def test_shipped_constants_twenty_frames(srukf, synth):
    """Shipped a1..a4 = 8, N = 8, seed 3, 20 frames of predict -> update_joint: no frame flagged (where the reference's form clamps from frame 2 on and is
    singular at frame 4), the pose finite and on np_joint's trajectory within the shipped-constant bound."""
    p = synth.default_params()
    sc = synth.make_scene(8, 20, seed=3, p=p)
    f, _ = start(srukf, sc)
    g = J.make_filter(synth, sc, p)
    tx, tp = tol(synth, "shipped")
    worst = [0.0, 0.0]
    for t in range(20):
        f.predict_motion(sc["odo"][t], sc["odo"][t + 1]); f.predict_measurement(); f.update_joint(sc["z"][t], sc["matched"][t])
        assert f.clamp_info() == (-1, -1), t
        g.predict_motion(sc["odo"][t], sc["odo"][t + 1]); g.predict_measurement(); g.update_joint(sc["z"][t], sc["matched"][t])
        pose, P4 = f.get_robot()
        assert np.isfinite(pose).all() and np.isfinite(P4).all()
        worst = [max(worst[0], np.abs(pose - g.X[-4:]).max()), max(worst[1], np.abs(P4 - (g.S.T @ g.S)[-4:, -4:]).max())]
    f.close()
    print("shipped constants, 20 frames: pose |dX| %.2e |dP| %.2e (bounds %.1e %.1e); theta clamps of the restatement %d" % (*worst, tx, tp, g.stats["theta"]))
    assert g.stats["theta"] == 0
    assert worst[0] <= tx and worst[1] <= tp


def test_displaced_pose(srukf, synth):
    """Pose displaced 0.1 m (innovations ~ 25 px): the joint update brings the error down on the device, to np_joint's value within 1e-9 m; BATCHED drives it up"""
    sc, X0, S0 = J.displaced_scene(synth)
    g = J.NpJointFilter(8, sc["params"], synth); g.set_state(X0, S0)
    g.predict_motion(sc["odo"][0], sc["odo"][1]); g.predict_measurement(); g.update_joint(sc["z"][0], sc["matched"][0])
    err = {}
    for name in ("joint", "batched"):
        f, _ = start(srukf, sc, X0=X0, S0=S0)
        f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement()
        before = np.linalg.norm(f.get_robot()[0][:2] - sc["odo"][1, :2])
        f.update_joint(sc["z"][0], sc["matched"][0]) if name == "joint" else f.update(sc["z"][0], sc["matched"][0], mode=srukf.UPDATE_BATCHED)
        pose = f.get_robot()[0]; f.close()
        err[name] = (before, np.linalg.norm(pose[:2] - sc["odo"][1, :2]), pose)
        print("%s: pose error %.4f -> %.4f m" % (name, err[name][0], err[name][1]))
    assert err["joint"][1] < 0.05 * err["joint"][0] and err["batched"][1] > err["batched"][0]
    assert np.abs(err["joint"][2] - g.X[-4:]).max() <= 1e-9


def test_default_path_untouched_and_fast_path_resumes(srukf, synth):
    """N = 50, 4 frames.  Twin a: frame 2 is predicted on the fast path and updated with update_joint (rewound, predicted again on the slow form); twin b never
    calls the new entry and is bit for bit a third filter that runs BATCHED throughout.  Behind the joint frame a takes the fast path again."""
    sc = synth.make_scene(50, 4, seed=5)
    fs = [srukf.Filter(50, sc["params"]) for _ in range(3)]
    for f in fs: f.set_state(sc["X0"], sc["S0"])
    a, b, c = fs
    counts = []
    for t in range(4):
        for f in fs:
            f.predict_motion(sc["odo"][t], sc["odo"][t + 1]); f.predict_measurement()
            if f is a and t == 2: f.update_joint(sc["z"][t], sc["matched"][t])
            else: f.update(sc["z"][t], sc["matched"][t], mode=srukf.UPDATE_BATCHED)
        counts.append((a.debug_get("step_fast"), a.debug_get("step_slow")))
    Xa, Sa = a.get_state(); Xb, Sb = b.get_state(); Xc, Sc = c.get_state()
    nb = (b.debug_get("step_fast"), b.debug_get("step_slow"))
    for f in fs: f.close()
    print("a: (fast, slow) per frame", counts, " b:", nb)
    assert counts[1][0] == counts[0][0] + 1                              # frame 1 ran on the fast path
    assert counts[2] == (counts[1][0], counts[1][1] + 1)                 # the joint frame: the slow form
    assert counts[3] == (counts[2][0] + 1, counts[2][1])                 # ... and the fast path again behind it
    assert Xb.tobytes() == Xc.tobytes() and Sb.tobytes() == Sc.tobytes() and nb[0] >= 3
    assert np.abs(Xa - Xb).max() < 1e-6 and np.isfinite(Sa).all()        # (healthy scene: the two forms agree closely; they are not the same update)


def test_storage_and_argument_errors(srukf, synth):
    sc = _scene(synth, 8, "scene")
    eps32 = float(np.finfo(np.float32).eps)
    X0, S0 = sc["X0"].astype(np.float32).astype(np.float64), np.triu(sc["S0"]).astype(np.float32).astype(np.float64)
    res = []
    for storage in (srukf.STORAGE_F64, srukf.STORAGE_F32):
        f = srukf.Filter(8, sc["params"]); f.set_storage(storage); f.set_state(X0, S0)
        f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement(); f.update_joint(sc["z"][0], sc["matched"][0])
        res.append(f.get_state()); f.close()
    (X, S), (X32, S32) = res
    np.testing.assert_allclose(X32, X, rtol=eps32, atol=1e-9)
    bound = eps32 * (np.abs(S32).T @ np.abs(S32)) * 1.5 + 1e-11          # every entry of S rounded to float (tests/test_gpu_parity_r2.py)
    assert (np.abs(S32.T @ S32 - S.T @ S) <= bound).all()
    assert np.array_equal(S32, S32.astype(np.float32).astype(np.float64))
    f = srukf.Filter(8, sc["params"]); f.set_state(sc["X0"], sc["S0"])
    z, m = sc["z"][0], sc["matched"][0]
    with pytest.raises(srukf.SrukfError) as e: f.update_joint(z, m)                       # before predict_measurement
    assert e.value.rc == -5
    f.predict_motion(sc["odo"][0], sc["odo"][1])
    with pytest.raises(srukf.SrukfError) as e: f.update_joint(z, m)
    assert e.value.rc == -5
    f.predict_measurement()
    with pytest.raises(srukf.SrukfError) as e: f.update_joint(z, m, reorder=7)
    assert e.value.rc == -1
    with pytest.raises(srukf.SrukfError) as e: f.update_joint(z, m, reorder=srukf.NEED_REORDER)   # no landmarks armed
    assert e.value.rc == -5
    Xp, Sp = f.get_state()
    f.update_joint(z, np.zeros(8, dtype=np.int32))                                              # no match: no-op (SLAM.cpp:2050-2051)
    Xn, Sn = f.get_state()
    assert np.array_equal(Xp, Xn) and np.array_equal(Sp, Sn)
    f.close()
    f = srukf.Filter(8, sc["params"]); f.debug_allow_mixed(1); f.set_storage(srukf.STORAGE_F32_MIXED); f.set_state(X0, S0)
    f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement()
    with pytest.raises(srukf.SrukfError) as e: f.update_joint(z, m)
    assert e.value.rc == -6
    f.close()


def test_facade_replay_with_joint_update(tmp_path, synth):
    """cslam_replay joint=1 (CSLAM::jointUpdate) on an N = 20 sequence: the facade's trajectory is np_joint's within the per-frame bounds, no update flagged;
    without the argument (and with joint=0) the program prints what it always printed, the timing at the end of the last line aside."""
    import os
    import subprocess
    from test_gpu_facade import REPLAY, _write_inputs
    assert os.path.exists(REPLAY), "run __graft_entry__.build() first"
    p = synth.scene_params()
    F = 12
    sc = synth.make_scene(20, F, seed=3, p=p)
    tmp = str(tmp_path)
    _write_inputs(tmp, sc, p)
    runs = {}
    for name, extra in (("plain", []), ("joint0", ["joint=0"]), ("joint1", ["joint=1"])):
        out = subprocess.run([REPLAY, f"{tmp}/scene.bin", f"{tmp}/odo.txt", f"{tmp}/RobotPath_{name}.txt", f"{tmp}/traj_{name}.bin", "batched"] + extra,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        runs[name] = (out.stdout, open(f"{tmp}/traj_{name}.bin", "rb").read(), open(f"{tmp}/RobotPath_{name}.txt", "rb").read())
    strip = lambda s: [l.split("  total ")[0] for l in s.splitlines()]
    assert strip(runs["plain"][0]) == strip(runs["joint0"][0]) and runs["plain"][1:] == runs["joint0"][1:]
    assert "joint" not in runs["plain"][0] and runs["joint1"][0].splitlines()[-1] == "joint flagged 0"
    assert strip(runs["joint1"][0])[:-1] == strip(runs["plain"][0])           # same frames, landmarks, predicts, matches
    traj = np.frombuffer(runs["joint1"][1]).reshape(F, 8)
    ref = J.make_filter(synth, sc).run_joint(sc)
    dX, dP = np.abs(traj[:, :4] - ref[:, :4]).max(), np.abs(traj[:, 4:] - ref[:, 4:]).max()
    print("facade joint=1, 12 frames: |dX| %.2e |dP| %.2e; against the default run %.2e m" % (dX, dP, np.abs(traj[:, :4] - np.frombuffer(runs["plain"][1]).reshape(F, 8)[:, :4]).max()))
    assert dX <= TOL_X and dP <= TOL_P
    assert traj.tobytes() != runs["plain"][1]


def test_facade_ransac_branch_routes_through_the_joint_update(tmp_path, synth):
    """CSLAM::isUseRANSAC with jointUpdate: on a clean N = 20 sequence every match is a low-innovation inlier (tests/test_gpu_ransac.py), so the inlier update is one
    joint update over the same matches as the plain branch's — and the consensus changes nothing of the filter: the two joint runs print the same trajectory, bit for bit."""
    import os
    import struct
    import subprocess
    from test_gpu_facade import REPLAY, _write_inputs
    assert os.path.exists(REPLAY), "run __graft_entry__.build() first"
    p = synth.scene_params()
    N, F = 20, 8
    sc = synth.make_scene(N, F, seed=5, p=p)
    tmp = str(tmp_path)
    _write_inputs(tmp, sc, p)
    traj = {}
    for name, extra in (("joint", ["joint=1"]), ("both", ["joint=1", f"ransac={tmp}/ransac.bin"]), ("batched", [])):
        out = subprocess.run([REPLAY, f"{tmp}/scene.bin", f"{tmp}/odo.txt", f"{tmp}/RobotPath_{name}.txt", f"{tmp}/traj_{name}.bin", "batched"] + extra,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        if extra: assert out.stdout.splitlines()[-1] == "joint flagged 0"
        traj[name] = open(f"{tmp}/traj_{name}.bin", "rb").read()
    raw, off = open(f"{tmp}/ransac.bin", "rb").read(), 0
    for _ in range(F):
        lo, hi, n = struct.unpack_from("iii", raw, off); off += 12 + 6 * n
        assert (lo, hi, n) == (N, 0, N)
    assert traj["both"] == traj["joint"] and traj["joint"] != traj["batched"]
