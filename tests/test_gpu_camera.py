"""Every copy of the camera model on the device under cameras where each of its terms counts (tests/cameras.py: k2 != 0, f1 != f2, image_w != 640, odd and
small Newton counts): srukf_project bit for bit against its Python restatement and against the oracle and a 40-digit reference; the frame paths (step-wise
calls, the staged replay and the switches that choose which kernel projects), the landmark initialisation, the association's warp, the RANSAC and the archive
kernels against the oracle and its numpy restatements.  tests/test_camera_cpu.py holds the references to each other and asserts the scenes' preconditions."""
import functools

import numpy as np
import pytest

import cameras as C
import np_archive
import np_ransac
import test_gpu_archive as TA
import test_gpu_ransac as TR
from test_camera_cpu import MP_BOUND
from test_gpu_detect import texture
from test_gpu_parity import _texture

pytestmark = pytest.mark.gpu

TOL_X, TOL_P, TOL_H = 1e-9, 1e-11, 1e-8
FRAMES = 4


# ---- a. srukf.project on general points --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.NAMES)
def test_project_matches_oracle_and_mpmath(srukf, oracle, synth, name):
    """4096 general points (landmarks to 200 px from the principal point) against oracle.project(early_exit=0) at 1e-10, the first 256 against the mpmath
    projection at the oracle's measured distance from it (test_camera_cpu.MP_BOUND) + 1e-10.  A point is left out only next to a threshold."""
    p, feat, pos, psi, err = C.general(synth, name)
    keep = ~C.near_threshold(p, feat, pos, psi, err)
    assert (~keep).sum() <= 0.01 * len(keep)
    uv = srukf.project(p, feat, pos, psi, err)
    ref = oracle.project(p, feat, pos, psi, err, early_exit=0)
    d = np.abs(uv - ref)[keep].max()
    dm = np.abs(uv[:256] - C.mp_reference(name))[keep[:256]].max()
    print(f"camera {name}: |device - oracle| max = {d:.3e} px, |device - mpmath| max = {dm:.3e} px, {(~keep).sum()} points left out")
    np.testing.assert_allclose(uv[keep], ref[keep], rtol=0, atol=1e-10)
    assert dm <= MP_BOUND + 1e-10
    if name in ("barrel_neg", "small_img"):
        border, oov = C.branches(p, feat, pos, psi, err)
        assert (border & keep).sum() >= 40                       # zeroed by coordinatesCamera2Image
        # (the view test of distortOnePointRW can fail only where d < 1: test_camera_cpu.test_general_points_meet_the_gpu_test_conditions)
        if name == "barrel_neg": assert (oov & keep).sum() >= 40 and np.all(uv[oov & keep] == 0.0)


# ---- b. srukf.project bit for bit ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", C.NEWTON_KS)
@pytest.mark.parametrize("name", C.NAMES)
def test_project_equals_restatement_bit_for_bit(srukf, synth, name, K):
    """1024 pixels through inputs that make the front of srukf_project exact, newton_iters = K: both outputs equal tail(shortcut=False) in every bit.  Sees the
    parity rule of the 2-cycle exit, the loop count, every k2 term and the border comparisons at, just below and just above 10, image_w - 10, image_h - 10."""
    p = C.camera(synth, name, newton_iters=K)
    err = C.exact_errs(p, C.EXACT_N, seed=C.EXACT_SEED)
    ux, uy, zeroed = C.exact_seen(p, err)
    assert 8 <= zeroed.sum() <= 100
    ref = C.tail_full_table(p, ux, uy)[K]
    feat, pos, psi = C.exact_inputs(err)
    uv = srukf.project(p, feat, pos, psi, err)
    np.testing.assert_array_equal(uv[:, 0], ref[:, 0])
    np.testing.assert_array_equal(uv[:, 1], ref[:, 1])


# ---- c. frames against the oracle ------------------------------------------------------------------------------------------------------------------------------

def _device_Z(f):
    mp = (2 * f.N + 63) // 64 * 64
    return f.debug_copy("Z", f.L * mp).reshape(f.L, mp)[:, :2 * f.N].T


def _defined(S, p, N, Na):
    """bool[2N, L]: the entries of the device's Z that a frame from factor S defines.  The rank-aware forms (n >= 128) project a structurally null direction
    (a row sqrt(EPSILON) e_i of S) for its own landmark only; the rest of those two columns is neither written nor read (test_gpu_parity_r3 holds the two
    tail forms to each other on the same set).  Smaller maps, and a first frame from the joint initialisation's zero rows, project everything."""
    n = 6 * N + 4
    ok = np.ones((2 * N, 2 * Na + 1), dtype=bool)
    if n < 128: return ok
    for i in range(2, n - 4):
        if np.count_nonzero(S[i]) == 1 and S[i, i] == np.sqrt(p["epsilon"]):
            for c in (1 + i, 1 + Na + i):
                ok[:, c] = False; ok[2 * (i // 6):2 * (i // 6) + 2, c] = True
    return ok


def _stepwise(srukf, oracle, sc, mode, hint=False):
    """FRAMES frames through the step-wise calls beside the oracle: h, visibility, X and P frame by frame against an oracle that runs on its own.  The pixels of
    every sigma point are compared with Oracle.Z() of a second oracle that starts each frame from the device's own factor: the sigma points are X +- gamma S_i,
    and S is not unique where P is (row signs, the null space of a joint initialisation), so after the first frame two correct filters hold different points."""
    N, p = sc["N"], sc["params"]
    f = srukf.Filter(N, p); f.set_state(sc["X0"], sc["S0"])
    o = oracle.Oracle(N, p); o.set_state(sc["X0"], sc["S0"])
    oz = oracle.Oracle(N, p)
    X, S = sc["X0"], sc["S0"]
    worst = 0.0
    for t in range(FRAMES):
        oz.set_state(X, S); oz.predict_motion(sc["odo"][t], sc["odo"][t + 1]); oz.predict_measurement()
        f.predict_motion(sc["odo"][t], sc["odo"][t + 1]); o.predict_motion(sc["odo"][t], sc["odo"][t + 1])
        if hint: f.predict_motion_next(sc["odo"][t + 1], sc["odo"][t + 2])
        h, Si, vis = f.predict_measurement()
        ho, Sio, viso = o.predict_measurement()
        Zo = oz.Z()
        assert np.all(Zo != 0.0) and np.all(o.Z() != 0.0)        # (the scene's precondition: no sigma point at a border)
        assert np.array_equal(vis, viso)
        np.testing.assert_allclose(h, ho, rtol=0, atol=TOL_H)
        ok = _defined(S, p, N, f.Na)
        assert ok.mean() > 0.4 and ok[:, 0].all() and ok[:, f.n - 3:1 + f.Na].all() and ok[:, f.Na + f.n - 3:].all()      # centre, robot and noise directions in full
        dz = np.abs(_device_Z(f) - Zo)[ok].max()
        worst = max(worst, dz)
        assert dz <= TOL_H, (t, dz)
        f.update(sc["z"][t], sc["matched"][t], mode=mode); o.update(sc["z"][t], sc["matched"][t], 1, 0, mode)
        X, S = f.get_state(); Xo, So = o.get_state()
        np.testing.assert_allclose(X, Xo, rtol=0, atol=TOL_X)
        np.testing.assert_allclose(S.T @ S, So.T @ So, rtol=0, atol=TOL_P)
    print(f"camera frames N={N} mode={mode}: max|dZ| = {worst:.3e} px")
    assert o.clamp_stats()["theta"] == 0
    f.close(); o.close(); oz.close()


@pytest.mark.parametrize("mode", [0, 1], ids=["sequential", "batched"])
@pytest.mark.parametrize("name", C.NAMES)
def test_stepwise_frames_n8(srukf, oracle, synth, name, mode):
    assert (srukf.UPDATE_SEQUENTIAL, srukf.UPDATE_BATCHED) == (0, 1) == (oracle.Oracle.SEQUENTIAL, oracle.Oracle.BATCHED)
    _stepwise(srukf, oracle, C.scene(synth, name, *C.SCENES[0]), mode)


@functools.lru_cache(maxsize=None)
def _oracle_states_n40(name):
    """the oracle's state after each of FRAMES batched frames of the N = 40 scene (shared between the staged cases of a camera, never changed)"""
    import __graft_entry__ as ge
    from oracle import oracle as O
    sc = C.scene(ge.load_package().synth, name, *C.SCENES[1])
    o = O.Oracle(40, sc["params"]); o.set_state(sc["X0"], sc["S0"])
    out = []
    for t in range(FRAMES):
        o.predict_motion(sc["odo"][t], sc["odo"][t + 1]); o.predict_measurement()
        assert np.all(o.Z() != 0.0)
        o.update(sc["z"][t], sc["matched"][t], 1, 0, O.Oracle.BATCHED)
        Xo, So = o.get_state()
        out.append((Xo, So.T @ So))
    assert o.clamp_stats()["theta"] == 0
    o.close()
    return sc, out


STAGED = [("default", None), ("fused_motion_0", ("fused_motion", 0)), ("fused_motion_1", ("fused_motion", 1)), ("tail_fuse_0", ("tail_fuse", 0)),
          ("pxy2_0", ("pxy2", 0)), ("rank_aware_0", None)]


@pytest.mark.parametrize("variant,switch", STAGED, ids=[v for v, _ in STAGED])
@pytest.mark.parametrize("name", ["k2_strong", "nonsquare", "odd_iters"])
def test_staged_frames_n40(srukf, synth, name, variant, switch):
    """The staged replay at N = 40 ("fused tail" plan: k_project_motion, k_project_table, k_rank_expand's tail project) and under each switch that chooses
    another projecting kernel, frame by frame against the oracle."""
    sc, ref = _oracle_states_n40(name)
    f = srukf.Filter(40, sc["params"])
    if variant == "rank_aware_0": f.set_rank_aware(0)
    if switch: f.debug_set(*switch)
    f.set_state(sc["X0"], sc["S0"]); f.stage_sequence(sc["odo"], sc["z"], sc["matched"])
    for t in range(FRAMES):
        f.run_frames(t, 1)
        X, S = f.get_state()
        np.testing.assert_allclose(X, ref[t][0], rtol=0, atol=TOL_X)
        np.testing.assert_allclose(S.T @ S, ref[t][1], rtol=0, atol=TOL_P)
    assert f.debug_get("clamp_rows") == 0 and f.debug_get("gmw_aborts") == 0
    if variant == "default": assert f.debug_get("plan_fuse") == 1
    f.close()


@pytest.mark.parametrize("name", ["k2_strong", "nonsquare", "odd_iters"])
def test_stepwise_equals_staged_n40(srukf, oracle, synth, name):
    """The step-wise calls at N = 40 (the replay's own launch sequence cut at the association step) against the oracle frame by frame, h, visibility and all
    sigma-point pixels included, and bit for bit against the staged replay, as test_gpu_parity_r5.test_step_api_equals_staged_replay holds them."""
    sc, _ = _oracle_states_n40(name)
    _stepwise(srukf, oracle, sc, srukf.UPDATE_BATCHED, hint=True)
    # from the state after the first staged frame, as there: a run's first frame from the joint initialisation's zero rows takes another launch sequence
    w = srukf.Filter(40, sc["params"]); w.set_state(sc["X0"], sc["S0"]); w.stage_sequence(sc["odo"], sc["z"], sc["matched"]); w.run_frames(0, 1)
    X1, S1 = w.get_state(); w.close()
    a = srukf.Filter(40, sc["params"]); a.set_state(X1, S1); a.stage_sequence(sc["odo"], sc["z"], sc["matched"])
    a.run_frames(1, FRAMES)
    Xa, Sa = a.get_state(); a.close()
    b = srukf.Filter(40, sc["params"]); b.set_state(X1, S1)
    for t in range(1, 1 + FRAMES):
        b.predict_motion(sc["odo"][t], sc["odo"][t + 1]); b.predict_motion_next(sc["odo"][t + 1], sc["odo"][t + 2])
        b.predict_measurement(); b.update(sc["z"][t], sc["matched"][t])
    assert b.debug_get("step_fast") == FRAMES and b.debug_get("step_slow") == 0
    Xb, Sb = b.get_state(); b.close()
    assert np.array_equal(Xa, Xb) and np.array_equal(Sa, Sb)


# ---- d. landmark initialisation ----------------------------------------------------------------------------------------------------------------------------------

def _uv(p, K, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(30, p["image_w"] - 30, K), rng.uniform(30, p["image_h"] - 30, K)])


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("name", ["default", "k2_strong", "barrel_neg", "nonsquare", "small_img"])
def test_add_landmarks_from_empty_map(srukf, oracle, synth, name, K):
    """srukf_augment.hip's undistortion and pixel-to-angles front against oracle.joint_init, pixels over the whole image (30 px inside)."""
    p = C.camera(synth, name)
    uv = _uv(p, K, 50 + K)
    f = srukf.Filter(0, p)
    X4, S4 = f.get_state()
    Xo, So = oracle.joint_init(p, X4, S4, uv)
    f.add_landmarks(uv)
    X, S = f.get_state()
    assert (f.N, f.n) == (K, 6 * K + 4) and np.all(np.tril(S, -1) == 0.0)
    np.testing.assert_allclose(X, Xo, rtol=0, atol=1e-13)
    np.testing.assert_allclose(S.T @ S, So.T @ So, rtol=0, atol=1e-12)
    f.close()


REORDER_SEED = 58              # with the oracle on the CPU: every sigma point of the frame after the initialisation is in view


def test_add_landmarks_then_need_reorder_frame_nonsquare(srukf, oracle, synth):
    """Eight landmarks from the empty map under nonsquare, then the frame the reference runs right after: KalmanUpdate with NEED_REORDER, K_new = 8."""
    p = C.camera(synth, "nonsquare")
    K = 8
    uv = _uv(p, K, REORDER_SEED)
    odo = synth.figure8_odometry(2)
    f = srukf.Filter(0, p)
    X4, S4 = f.get_state()
    Xo, So = oracle.joint_init(p, X4, S4, uv)
    f.add_landmarks(uv)
    X, S = f.get_state()
    np.testing.assert_allclose(X, Xo, rtol=0, atol=1e-12)
    np.testing.assert_allclose(S.T @ S, So.T @ So, rtol=0, atol=1e-11)
    o2 = oracle.Oracle(K, p); o2.set_state(X, S)
    f.predict_motion(odo[0], odo[1]); h, Si, vis = f.predict_measurement()
    o2.predict_motion(odo[0], odo[1]); ho, Sio, viso = o2.predict_measurement()
    assert np.all(o2.Z() != 0.0) and viso.all() and np.array_equal(vis, viso)
    np.testing.assert_allclose(h, ho, rtol=0, atol=1e-8)
    rng = np.random.default_rng(3)
    z = h + rng.normal(0, 0.5, h.shape); m = np.asarray(vis, dtype=np.int32)
    f.update(z, m, reorder=srukf.NEED_REORDER, mode=srukf.UPDATE_SEQUENTIAL)
    o2.update(z, m, reorder=oracle.Oracle.NEED_REORDER, k_new=K, mode=oracle.Oracle.SEQUENTIAL)
    X2, S2 = f.get_state(); Xo2, So2 = o2.get_state()
    np.testing.assert_allclose(X2, Xo2, rtol=0, atol=1e-8)
    np.testing.assert_allclose(S2.T @ S2, So2.T @ So2, rtol=0, atol=1e-9)
    f.close()


# ---- e. association bytes ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["k2_strong", "nonsquare", "small_img"])
def test_data_association_matches_oracle(srukf, oracle, synth, name):
    """test_gpu_parity.test_data_association_matches_oracle's construction with N = 12: dev_distort, dev_undistort and the warp's K matrix of srukf_assoc.hip
    decide bytes of the warped template; they must be the oracle's where k2 != 0 and f1 != f2, on a 480 x 400 frame too."""
    p = C.camera(synth, name)
    N, W, H = 12, int(p["image_w"]), int(p["image_h"])
    sc = synth.make_scene(N, 3, seed=13, p=p)
    rng = np.random.default_rng(2)
    T = _texture(rng, H, W)
    f = srukf.Filter(N, p); f.set_state(sc["X0"], sc["S0"])
    pose0 = sc["X0"][-4:].copy()
    R0 = np.array([[np.cos(pose0[3]), -np.sin(pose0[3]), 0], [np.sin(pose0[3]), np.cos(pose0[3]), 0], [0, 0, 1.0]])
    f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement(); f.update(sc["z"][0], sc["matched"][0])
    f.predict_motion(sc["odo"][1], sc["odo"][2]); h, Si, vis = f.predict_measurement()
    shift = (2, -1)
    frame = np.roll(T, (shift[1], shift[0]), axis=(0, 1))
    init_px, patches = [], []
    for k in range(N):
        ipx = h.reshape(N, 2)[k] - np.array(shift) + rng.uniform(-1.5, 1.5, 2)
        cu, cv = int(round(ipx[0])), int(round(ipx[1]))
        assert 20 <= cu < W - 20 and 20 <= cv < H - 20
        patch = T[cv - 10:cv + 11, cu - 10:cu + 11].copy()
        init_px.append(ipx); patches.append(patch)
        if k != 5: f.set_landmark_appearance(k, patch, R0, pose0[:3], ipx)
    X, S = f.get_state()
    xyz, _ = f.get_landmarks_cartesian()
    z, m, cr = f.associate(frame)
    assert m[5] == 0 and cr[5] == 0.0
    assert vis.sum() >= N - 1
    pose = X[-4:]
    Rc = np.array([[np.cos(pose[3]), -np.sin(pose[3]), 0], [np.sin(pose[3]), np.cos(pose[3]), 0], [0, 0, 1.0]])
    for leg in (0, 1):
        if leg == 1:                                             # created at the current pose: the identity view, every warped coordinate next to an integer
            for k in range(N): f.set_landmark_appearance(k, patches[k], Rc, pose[:3], init_px[k])
            z, m, cr = f.associate(frame)
        R, t = (R0, pose0[:3]) if leg == 0 else (Rc, pose[:3])
        for k in range(N):
            if (leg == 0 and k == 5) or not vis[k]:
                assert m[k] == 0
                continue
            mp_o = oracle.warp_patch(p, pose, R, t, init_px[k], xyz[k], h.reshape(N, 2)[k], patches[k], np.zeros((17, 17), dtype=np.uint8))
            mp_d = f.get_match_patch(k)
            assert np.array_equal(mp_o, mp_d), (leg, k, np.abs(mp_o.astype(int) - mp_d.astype(int)).max())
            ok, best, loc = oracle.associate_one(p, frame, h.reshape(N, 2)[k], Si.reshape(N, 4)[k], mp_o)
            assert abs(best - cr[k]) < 1e-9
            assert bool(m[k]) == ok
            if ok: np.testing.assert_allclose(z[2 * k:2 * k + 2], loc, rtol=0, atol=1e-9)
        if leg == 1: assert m.sum() >= N // 2                  # the identity view finds its patches
    f.close()


# ---- f. the RANSAC and archive kernels ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["nonsquare", "k2_strong"])
def test_ransac_consensus_and_repredict(srukf, oracle, synth, name):
    """k_ransac's own marshalling of the parameter struct: the consensus against np_ransac.consensus (test_gpu_ransac's helpers and tolerance), then
    srukf_repredict_measurement and a second update against the oracle (test_repredict_and_second_update_equal_oracle's construction and bounds).  N = 12."""
    N, seed, F0 = 12, 5, TR.F0
    p = C.camera(synth, name)
    sc = synth.make_scene(N, F0 + 3, seed=seed, p=p)
    X3, S3 = TR._warm_state(srukf, sc, N, p)
    o = oracle.Oracle(N, p); o.set_state(X3, S3)
    o.predict_motion(sc["odo"][F0], sc["odo"][F0 + 1])
    ho, Sio, viso = o.predict_measurement()
    assert viso.all() and np.all(o.Z() != 0.0)
    f = srukf.Filter(N, p); f.set_state(X3, S3)
    h, Si, vis = TR._predict(f, sc, F0, 0)
    assert np.array_equal(vis, viso)
    for kind in TR.KINDS:
        z, m, moved = TR.make_z(sc, F0, ho, viso, kind, seed)
        res = np_ransac.consensus(oracle, o, p, z, m)
        inl, votes, dist, best = f.ransac_consensus(z, m, 8.0)
        err, share = np_ransac.compare(res, inl, votes, dist, best, 8.0, TR.DIST_TOL)
        print(f"camera {name} ransac {kind}: best={best} votes={votes[best]} max|ddist|={err:.3e}")
        assert share == 0.0 and err <= TR.DIST_TOL
        assert kind == "near" or set(np.flatnonzero(inl)).isdisjoint(moved)
    z, m = sc["z"][F0], sc["matched"][F0].astype(np.int32)
    m1, m2 = m.copy(), m.copy()
    m1[1::2] = 0; m2[0::2] = 0
    f.update(z, m1)
    Xp, Sp = f.get_state()
    h2, Si2, vis2 = f.repredict_measurement()
    o2 = oracle.Oracle(N, p); o2.set_state(Xp, Sp)
    o2.predict_motion(np.zeros(3), np.zeros(3))
    h2o, Si2o, vis2o = o2.predict_measurement()
    assert np.array_equal(vis2, vis2o) and np.all(o2.Z() != 0.0)
    assert np.abs(h2 - h2o).max() < 1e-8 and np.abs(np.abs(Si2) - np.abs(Si2o)).max() < 1e-9
    f.update(z, m2); o2.update(z, m2, 1, 0, oracle.Oracle.BATCHED)
    X, S = f.get_state(); Xo, So = o2.get_state()
    assert np.abs(X - Xo).max() <= 1e-9 and np.abs(S.T @ S - So.T @ So).max() <= 1e-11
    f.close()


@pytest.mark.parametrize("name", ["nonsquare", "k2_strong"])
def test_archive_predict(srukf, oracle, synth, name):
    """k_archive_predict's own marshalling: h, Si^T Si and visible of archive_search against np_archive.predict for L = 8 records of a running filter, between
    predict and update and after the update (test_gpu_archive.test_predict_equals_restatement's construction and tolerances)."""
    N, seed, F0, L = 20, 11, TA.F0, 8
    p = C.camera(synth, name)
    sc = synth.make_scene(N, F0 + 3, seed=seed, p=p)
    X3, S3 = TA._warm_state(srukf, sc, N, p)
    f = srukf.Filter(N, p); f.set_state(X3, S3)
    img = texture(4, H=int(p["image_h"]), W=int(p["image_w"]))
    ks = [0, 3, 5, 8, 12, 14, 17, 19]
    TA._predict(f, sc, F0, 0)
    for phase in ("between", "after"):
        if phase == "after": f.update(sc["z"][F0], sc["matched"][F0])
        rec = TA.scene_records(f, ks)
        TA.set_archive(f, rec)
        assert f.archive_count() == L
        h, Si, vis, z, m, cr = f.archive_search(img)
        pose, P4 = f.get_robot()
        hr, Sir, visr, _, Z = np_archive.predict(oracle, p, rec["X6"], rec["S66"], pose, P4)
        assert all(np_archive.border_margin(p, Z[k]) > 1.0 for k in range(L))
        assert np.array_equal(vis, visr) and vis.all()
        dh = np.abs(h.reshape(L, 2) - hr).max()
        dp = np.abs(np.einsum("kab,kac->kbc", Si, Si) - np.einsum("kab,kac->kbc", Sir, Sir)).max()
        print(f"camera {name} archive predict {phase}: max|dh| = {dh:.3e} px, max|d(Si^T Si)| = {dp:.3e} px^2")
        assert dh <= TA.PRED_TOL_H and dp <= TA.PRED_TOL_P
    f.close()
