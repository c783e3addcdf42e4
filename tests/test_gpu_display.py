"""Display ellipsoids on the device (k_lm_ellipsoid behind srukf_get_landmarks_display / srukf_get_frame_view_display) against the restatement of the reference's
three functions on Python floats (tests/np_display.py): bit for bit, NaN positions included — the kernel runs the host facade's arithmetic operation for operation,
built without contraction, with correctly rounded fp64 sqrt and division.  (A NaN's sign and payload are not compared: what sqrt of a negative number sets there
differs between the device and an x86 host.)"""
import os
import struct
import subprocess

import numpy as np
import pytest

import np_display

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = os.path.join(ROOT, "cv-monoslam_amd", "cslam_replay.bin")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~na])


def restate(cov, eps):
    out = [np_display.ellipsoid(c.ravel().tolist(), eps) for c in cov]
    return (np.array([o[0] for o in out]).reshape(-1, 4), np.array([o[1] for o in out]).reshape(-1, 3), np.array([o[2] for o in out], dtype=np.int32))


def check_display(f, eps):
    """srukf_get_landmarks_display against srukf_get_landmarks_cartesian (xyz, cov) and against the restatement applied to the cov the same call returned."""
    xyz, cov, axis, sigma, rot = f.get_landmarks_display()
    xyz2, cov2 = f.get_landmarks_cartesian()
    assert same_bits(xyz, xyz2) and same_bits(cov, cov2)
    a, s, r = restate(cov, eps)
    assert np.array_equal(rot, r), (rot, r)
    assert same_bits(sigma, s), np.flatnonzero(~(sigma == s).all(axis=1))
    assert same_bits(axis, a), np.flatnonzero(~(axis == a).all(axis=1))
    return xyz, cov, axis, sigma, rot


def step(f, sc, t, hint=False):
    f.predict_motion(sc["odo"][t], sc["odo"][t + 1])
    if hint:
        f.predict_motion_next(sc["odo"][t + 1], sc["odo"][t + 2])
    f.predict_measurement()
    f.update(sc["z"][t], sc["matched"][t])


@pytest.mark.parametrize("K", [1, 2])
def test_jointly_initialised_landmarks(srukf, synth, K):
    """N = 1 and N = 2 from the joint initialisation of an empty map: the anchors are copies of the camera position, the state is rank deficient."""
    p = synth.scene_params()
    f = srukf.Filter(0, p)
    f.add_landmarks(np.array([[300.0, 200.0], [340.0, 260.0]][:K]))
    assert f.N == K
    xyz, cov, axis, sigma, rot = check_display(f, p["epsilon"])
    assert (rot >= 0).all() and np.abs(np.linalg.norm(axis, axis=1) - 1.0).max() < 1e-14
    f.close()


def test_n8_golden_frame(srukf, synth, golden):
    g = golden["g5_frame_n8"]
    p = synth.scene_params()
    f = srukf.Filter(8, p); f.set_state(g["X0"], g["S0"])
    f.predict_motion(g["odo"][0], g["odo"][1]); f.predict_measurement(); f.update(g["z"][0], g["matched"][0])
    xyz, cov, axis, sigma, rot = check_display(f, p["epsilon"])
    assert (rot >= 0).all()
    f.close()


def test_n65_second_workgroup_with_one_live_lane(srukf, synth):
    p = synth.scene_params()
    N = 65
    sc = synth.make_scene(N, 4, seed=17, p=p)
    f = srukf.Filter(N, p); f.set_state(sc["X0"], sc["S0"])
    for t in range(3):
        step(f, sc, t)
    xyz, cov, axis, sigma, rot = check_display(f, p["epsilon"])
    assert rot.shape == (N,) and (rot >= 0).all()
    f.close()


# 3 x 3 upper-triangular factors whose S^T S are the special inputs of tests/test_display_cpu.py (products chosen to be exact in binary64)
CRAFTED = {
    "diagonal": [[2.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, 0.0, 0.5]],
    "tie": [[1.0, 0.5, 0.5], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]],                         # cov[1][0] == cov[2][0] = 0.5 > cov[2][1] = 0.25: pivot (1, 0)
    "y<0": [[1.0, 0.5, 0.0], [0.0, 1.5, 0.0], [0.0, 0.0, 2.0]],                         # a00 = 1 < a11 = 2.5 with pivot (1, 0)
    "cond": [[1.0, 0.3, 0.2], [0.0, 1e-4, 0.5e-4], [0.0, 0.0, 1e-4]],                   # condition number ~1e8
    "rank1": [[0.345584192064786, 0.8216181435011584, 0.33043707618338714], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]],
}


def crafted_state(blocks, p):
    N = len(blocks); n = 6 * N + 4
    X, S = np.zeros(n), np.zeros((n, n))
    for k, B in enumerate(blocks):
        X[6 * k:6 * k + 6] = [0.1 * k, -0.2 * k, 1.0 + k, 0.0, 0.0, 1.0]                # theta = phi = 0, rho = 1
        S[6 * k:6 * k + 3, 6 * k:6 * k + 3] = B
    S[n - 4:, n - 4:] = np.diag([p["sigma_x"], p["sigma_y"], p["sigma_z"], p["sigma_theta"]])
    return X, S


def test_crafted_covariances_through_the_kernel(srukf, synth):
    """With theta = phi = 0 and rho = 1, S nonzero only in each landmark's xyz rows: cov is that block's S^T S, one exact product or short exact sum per entry."""
    p = synth.scene_params()
    names = list(CRAFTED)
    X, S = crafted_state([CRAFTED[k] for k in names], p)
    f = srukf.Filter(len(names), p); f.set_state(X, S)
    xyz, cov, axis, sigma, rot = check_display(f, p["epsilon"])
    for k, name in enumerate(names):
        B = np.array(CRAFTED[name])
        assert name == "cond" or same_bits(cov[k], B.T @ B), name    # ("cond": a three-term sum whose order is the kernel's)
    i = names.index
    assert rot[i("diagonal")] == 0 and axis[i("diagonal")].tolist() == [1.0, 0.0, 0.0, 0.0] and sigma[i("diagonal")].tolist() == [2.0, 3.0, 0.5]
    tr = []
    np_display.jacobi3(cov[i("tie")].ravel().tolist(), p["epsilon"], tr)
    assert cov[i("tie")][1, 0] == cov[i("tie")][2, 0] and tr[0] == (1, 0)
    assert rot[i("y<0")] == 1 and axis[i("y<0")][3] != 0.0
    assert rot[i("cond")] >= 2 and sigma[i("cond")].min() < 2e-4 and sigma[i("cond")].max() > 1.0
    assert np.isnan(sigma[i("rank1")]).tolist() == [False, False, True] and rot[i("rank1")] == 2     # the negative rounding residue of tests/test_display_cpu.py
    f.close()


def test_nan_covariance_returns_at_once(srukf, synth):
    """rho = NaN makes every entry of that landmark's cov NaN: no pivot, no rotation, the identity's quaternion, NaN semi-axes; its neighbour is untouched."""
    p = synth.scene_params()
    X, S = crafted_state([CRAFTED["tie"], CRAFTED["cond"]], p)
    X[5] = np.nan
    f = srukf.Filter(2, p); f.set_state(X, S)
    xyz, cov, axis, sigma, rot = f.get_landmarks_display()
    assert np.isnan(cov[0]).all() and rot[0] == 0 and axis[0].tolist() == [1.0, 0.0, 0.0, 0.0] and np.isnan(sigma[0]).all()
    a, s, r = restate(cov, p["epsilon"])
    assert same_bits(axis, a) and same_bits(sigma, s) and np.array_equal(rot, r) and not np.isnan(sigma[1]).any()
    f.close()


@pytest.mark.parametrize("path", ["fast", "fast_next", "slow", "f32"])
def test_frame_view_display_on_every_step_path(srukf, synth, path):
    """srukf_get_frame_view_display after every update of five frames: equal to srukf_get_frame_view on the shared outputs (asked AFTER it, so that on the fast
    path the view the update exported — live from the third frame on — is what it is compared with) and to srukf_get_landmarks_display on axis / sigma; and the
    states equal those of a filter that never calls it, bit for bit: the call is read-only and a pre-issued next-frame launch is not disturbed."""
    p = synth.scene_params()
    N, F = 60, 5
    sc = synth.make_scene(N, 10, seed=31, p=p)                   # (the scene of test_frame_view_rides_on_the_update_once_the_host_asks_for_it: every frame after the first is a fast-path frame)
    a, b = srukf.Filter(N, p), srukf.Filter(N, p)
    for f in (a, b):
        if path == "f32":
            f.set_storage(srukf.STORAGE_F32)
        f.set_state(sc["X0"], sc["S0"])
        if path == "slow":
            f.debug_set("step_fuse_export", 0)
    for t in range(F):
        for f in (a, b):
            step(f, sc, t, hint=path == "fast_next")
        cached_before = a.debug_get("view_hits")
        X, xyz, cov, axis, sigma, pose, P4 = a.get_frame_view_display()
        assert a.debug_get("view_hits") == cached_before         # (the exported view is neither used nor consumed)
        X2, xyz2, cov2, pose2, P42 = a.get_frame_view()
        assert same_bits(X, X2) and same_bits(xyz, xyz2) and same_bits(cov, cov2) and same_bits(pose, pose2) and same_bits(P4, P42)
        xyz3, cov3, axis3, sigma3, rot3 = check_display(a, p["epsilon"])
        assert same_bits(xyz, xyz3) and same_bits(cov, cov3) and same_bits(axis, axis3) and same_bits(sigma, sigma3)
        Xa, Sa = a.get_state(); Xb, Sb = b.get_state()
        assert same_bits(Xa, Xb) and same_bits(Sa, Sb), t
        assert same_bits(X, Xa)
    if path in ("fast", "fast_next"):
        assert a.debug_get("step_fast") == F - 1 and b.debug_get("step_fast") == F - 1
        assert a.debug_get("view_hits") >= 2                     # the comparisons above did meet a live exported view
    a.close(); b.close()


def test_after_map_changes_on_new_and_revived_contexts(srukf, synth):
    p = synth.scene_params()
    N = 24
    sc = synth.make_scene(N, 2, seed=5, p=p)
    f = srukf.Filter(N, p); f.set_state(sc["X0"], sc["S0"])
    step(f, sc, 0)
    ref = check_display(f, p["epsilon"])
    f.delete_landmark(3)                                         # a context of a size not seen before
    got = check_display(f, p["epsilon"])
    assert f.N == N - 1 and same_bits(got[0], np.delete(ref[0], 3, axis=0))
    f.add_landmarks(np.array([[300.0, 200.0]]))                  # N again: the first context, revived (its display buffer was used above)
    assert f.N == N
    check_display(f, p["epsilon"])
    f.delete_landmark(0)                                         # the second context, revived
    check_display(f, p["epsilon"])
    v = f.get_frame_view_display(); w = f.get_frame_view()
    assert all(same_bits(x, y) for x, y in zip((v[0], v[1], v[2], v[5], v[6]), w))
    f.close()


def test_null_pointers_and_empty_map(srukf, synth):
    import ctypes as C
    p = synth.scene_params()
    sc = synth.make_scene(8, 1, seed=2, p=p)
    f = srukf.Filter(8, p); f.set_state(sc["X0"], sc["S0"])
    L, h = f._lib, f._h
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    xyz, cov, axis, sigma, rot = f.get_landmarks_display()
    assert L.srukf_get_landmarks_display(h, None, None, None, None, None) == -1                  # SRUKF_ERR_BAD_ARG
    assert L.srukf_get_frame_view_display(h, None, None, None, None, None, None, None) == -1
    for want, pos in ((xyz, 0), (cov, 1), (axis, 2), (sigma, 3)):                                # each output alone
        out = np.full(want.shape, -7.0); args = [None] * 5; args[pos] = dp(out)
        assert L.srukf_get_landmarks_display(h, *args) == 0 and same_bits(out, want)
    r = np.full(8, -7, dtype=np.int32)
    assert L.srukf_get_landmarks_display(h, None, None, None, None, r.ctypes.data_as(C.POINTER(C.c_int))) == 0 and np.array_equal(r, rot)
    X, xyz2, cov2, axis2, sigma2, pose, P4 = f.get_frame_view_display()
    s = np.full((8, 3), -7.0); ps = np.full(4, -7.0)
    assert L.srukf_get_frame_view_display(h, None, None, None, None, dp(s), dp(ps), None) == 0 and same_bits(s, sigma) and same_bits(ps, pose)
    Xo = np.full(f.n, -7.0)
    assert L.srukf_get_frame_view_display(h, dp(Xo), None, None, None, None, None, None) == 0 and same_bits(Xo, X)
    assert same_bits(axis2, axis) and same_bits(sigma2, sigma)
    f.close()
    e = srukf.Filter(0, p)                                       # N == 0: SRUKF_OK, the robot's part of the frame view still arrives
    out = e.get_landmarks_display()
    assert [o.shape[0] for o in out] == [0, 0, 0, 0, 0]
    v = e.get_frame_view_display(); w = e.get_frame_view()
    assert same_bits(v[0], w[0]) and same_bits(v[5], w[3]) and same_bits(v[6], w[4]) and v[0].shape == (4,)
    e.close()


def _write_inputs(tmp, sc, p):
    with open(os.path.join(tmp, "scene.bin"), "wb") as f:
        f.write(struct.pack("ii", sc["N"], sc["F"]))
        f.write(np.array([p["a1"], p["a2"], p["a3"], p["a4"]], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(sc["X0"]).tobytes()); f.write(np.ascontiguousarray(sc["S0"]).tobytes()); f.write(np.ascontiguousarray(sc["z"]).tobytes())
    with open(os.path.join(tmp, "odo.txt"), "w") as f:
        for i, (x, y, th) in enumerate(sc["odo"]):
            f.write(f"{i + 1} : {0.1 * i:.3f} {float(x)!r} {float(y)!r} {float(th)!r}\n")


def test_facade_with_ellipsoids_on_the_device_writes_the_same_bytes(tmp_path, synth, golden):
    """cslam_replay, N = 20, 12 frames, display=<file> (%a): CSLAM::ellipsoidsOnDevice on and off give byte-identical display files (ID, xyz, cov, axis, sigma of
    every map node) and trajectories — the device's Jacobi iteration and quaternion are the host's, which is built without FMA contraction."""
    assert os.path.exists(REPLAY), "run __graft_entry__.build() first"
    p = synth.scene_params()
    N, F = 20, 12
    sc = synth.make_scene(N, 50, seed=int(golden["g6_trajectory_n20"]["seed"]), p=p)          # (the scene of tests/test_gpu_facade.py: no landmark leaves the map)
    sc = dict(sc, N=N, F=F, z=sc["z"][:F], odo=sc["odo"][:F + 1])
    tmp = str(tmp_path)
    _write_inputs(tmp, sc, p)
    outs = []
    for on in (0, 1):
        r = subprocess.run([REPLAY, f"{tmp}/scene.bin", f"{tmp}/odo.txt", f"{tmp}/RobotPath{on}.txt", f"{tmp}/traj{on}.bin", "batched",
                            f"ellipsoids={on}", f"display={tmp}/display{on}.txt"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append((open(f"{tmp}/display{on}.txt", "rb").read(), open(f"{tmp}/traj{on}.bin", "rb").read(), open(f"{tmp}/traj{on}.bin.features", "rb").read()))
    lines = outs[0][0].decode().splitlines()
    assert len(lines) == N and all(len(ln.split()) == 20 for ln in lines) and [int(ln.split()[0]) for ln in lines] == list(range(1, N + 1))
    vals = np.array([[float.fromhex(v) if v != "nan" else np.nan for v in ln.split()[1:]] for ln in lines])
    assert np.abs(np.linalg.norm(vals[:, 12:16], axis=1) - 1.0).max() < 1e-12 and np.nanmin(vals[:, 16:19]) > 0.0       # (the file holds ellipsoids, not zeros)
    if outs[0][0] != outs[1][0]:
        other = outs[1][0].decode().splitlines()
        names = ["x", "y", "z"] + [f"cov{e}" for e in range(9)] + ["axis.r", "axis.x", "axis.y", "axis.z", "sigma.x", "sigma.y", "sigma.z"]
        diff = [(ln.split()[0], names[e], a, b) for ln, lo in zip(lines, other) for e, (a, b) in enumerate(zip(ln.split()[1:], lo.split()[1:])) if a != b]
        assert not diff, diff[:8]
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
